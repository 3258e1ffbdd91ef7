"""What the blurred view costs, beside the plain view on the same windows and beside the chain a loader runs without the blur= stage
(DESIGN.md 4.23).
    python tools/blur_time.py [--out profiles/blur_time.txt] [--shape 512x1024:896] [--radii 0,2,4,8] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko).  n tiles of size^2 -> crop^2, float16 NCHW, timed by HIP events after a 0.25 s
spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections
(their min and max beside it).  The whole measurement is ONE GPU step: a child process under its own time limit; the parent never opens
the device.  Every yardstick is existing code, timed in the same process.  Per bound max_r (every tile blurred at that radius):
  (a) sl_normalize_blur_view beside sl_normalize_view (k_view, the jitter route) on the same windows
  (b) end to end, fits included: augment_batch(blur=, view=, tensor_format=) against augment_batch(tensor_format=) followed by a depthwise
      torch conv2d (replicate padding, the tile's own 17-tap kernel in float16) and torch crop / flip / rot90 with the same windows
The torch chain is another function (a float blur of the float16 tensor): it is the work a loader does today, not a reference for bits."""
import argparse
import statistics
import subprocess
import sys
import time


def radius_codes(r):
    """codes of radius exactly r: a binomial-like bell cut at r, its weights rounded and the remainder put into w_0"""
    import numpy as np
    if r == 0:
        return np.array([256] + [0] * 8, dtype=np.int32)
    sigma = r / 3.0
    g = np.exp(-np.arange(0, r + 1) ** 2 / (2.0 * sigma * sigma))
    g /= g[0] + 2.0 * g[1:].sum()
    w = np.zeros(9, dtype=np.int64)
    w[1:r + 1] = np.maximum(1, np.floor(256.0 * g[1:] + 0.5))
    w[0] = 256 - 2 * w[1:].sum()
    assert w[0] >= 0 and w[r] != 0
    return w.astype(np.int32)


def step(shape, radii, collections):
    sys.path.insert(0, ".")
    import numpy as np
    import torch
    import stainlib_amd
    from stainlib_amd import engine
    from tools.synth import synth_tiles

    def collection(fn, reps=20):
        """median ms of `reps` calls timed one by one, after a spin-up"""
        t_spin = time.perf_counter()
        while time.perf_counter() - t_spin < 0.25:
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)

    def timed(fn):
        ms = [collection(fn) for _ in range(collections)]
        return statistics.median(ms), min(ms), max(ms)

    def row(label, t):
        return "  %-100s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])

    n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    aug = stainlib_amd.GaussianBlurAugmenter((0.0, 8.0 / 3.0))
    rgb = synth_tiles(n, size, size, seed=9)
    dev = rgb.device
    M, maxC, status = engine.macenko_fit(rgb)
    assert int((status != 0).sum()) == 0
    Mt, ct = nz._target_on(dev)
    np.random.seed(3)
    ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=dev)
    view = stainlib_amd.TileView(crop)
    win = view.draw(n, size, size)
    dwin = torch.from_numpy(win).to(dev)
    tv = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
    tb = torch.empty_like(tv)
    full = torch.empty((n, 3, size, size), dtype=torch.float16, device=dev)
    ws = engine.Workspace()
    route = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct, alpha_beta=ab)
    lines = ["", "%d tiles of %d^2 -> %d^2, float16 NCHW (%.1f Mpx read, %.1f written), codes %s" % (
        n, size, crop, n * size * size / 1e6, n * crop * crop / 1e6, sorted(set(win[:, 2].tolist())))]
    tk = timed(lambda: engine.normalize_view(rgb, dwin, crop, 7, fmt=f16, out=tv, **route))
    lines.append(row("sl_normalize_view (k_view, jitter route) -> float16 NCHW", tk))

    def torch_view(x):
        """crop / flip / rot90 per dihedral code, the tiles of a code together"""
        for d in sorted(set(win[:, 2].tolist())):
            idx = np.nonzero(win[:, 2] == d)[0]
            wh, ww = (crop, crop)
            part = torch.stack([x[t, :, win[t, 0]:win[t, 0] + wh, win[t, 1]:win[t, 1] + ww] for t in idx])
            if d & 4:
                part = torch.flip(part, (3,))
            tb[torch.as_tensor(idx, device=dev)] = torch.rot90(part, d & 3, (2, 3))
        return tb

    for r in radii:
        codes_np = np.tile(radius_codes(r), (n, 1))
        codes = torch.from_numpy(codes_np).to(dev)
        tbv = timed(lambda: engine.normalize_blur_view(rgb, dwin, crop, 7, codes, max_r=r, fmt=f16, out=tb, **route))
        lines.append("")
        lines.append(row("max_r = %d  (a) sl_normalize_blur_view on the same windows, patches of %d" % (r, 64 - 2 * r), tbv))
        lines.append("    the blurred view takes %.2f of the plain view's time" % (tbv[0] / tk[0]))
        taps = torch.tensor(np.concatenate([codes_np[0][:0:-1], codes_np[0]]) / 256.0, dtype=torch.float16, device=dev)
        kh = taps.view(1, 1, 1, 17).repeat(3, 1, 1, 1)
        kv = taps.view(1, 1, 17, 1).repeat(3, 1, 1, 1)

        def chain():
            x = nz.augment_batch(rgb, ab, out=full, ws=ws, tensor_format=f16)[0]
            x = torch.nn.functional.pad(x, (8, 8, 8, 8), mode="replicate")
            x = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, kh, groups=3), kv, groups=3)
            return torch_view(x)

        def fused():
            return nz.augment_batch(rgb, ab, out=tb, ws=ws, tensor_format=f16, view=view, windows=dwin, blur=aug, blur_sigmas=codes_np)[0]

        tc, tf = timed(chain), timed(fused)
        lines.append(row("           (b) chain with the fit: augment_batch(tensor_format=) -> depthwise conv2d x 2 -> crop / flip / rot90", tc))
        lines.append(row("               fused with the fit: augment_batch(blur=, view=, tensor_format=)", tf))
        lines.append("    the fused call takes %.2f of the chain's time" % (tf[0] / tc[0]))
    print("device %s" % torch.cuda.get_device_name(0))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/blur_time.txt")
    ap.add_argument("--shape", default="512x1024:896")
    ap.add_argument("--radii", default="0,2,4,8")
    ap.add_argument("--collections", type=int, default=5)
    ap.add_argument("--step", help="(internal) the measurement, in this process")
    ap.add_argument("--step-timeout", type=int, default=480, help="seconds for the measurement")
    args = ap.parse_args()
    radii = [int(r) for r in args.radii.split(",")]
    if args.step:
        return step(args.step, radii, args.collections)
    r = subprocess.run([sys.executable, __file__, "--step", args.shape, "--radii", args.radii, "--collections", str(args.collections)],
                       capture_output=True, text=True, timeout=args.step_timeout)
    if r.returncode != 0:
        sys.exit("shape %s failed (exit status %d):\n%s" % (args.shape, r.returncode, (r.stdout + r.stderr)[-3000:]))
    dev, _, rest = r.stdout.partition("\n")
    text = "%s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up\n%s\n" % (
        dev, args.collections, rest.rstrip("\n"))
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
