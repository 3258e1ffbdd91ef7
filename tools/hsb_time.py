"""What the hue / saturation / brightness augmentation costs, beside its yardsticks and beside the chain a loader runs without the hsb=
stage.
    python tools/hsb_time.py [--out profiles/hsb_time.txt] [--shapes 512x1024:896,1250x512:448] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko).  Per shape (n tiles of size^2 -> crop^2, float16 NCHW), timed by HIP events after
a 0.25 s spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the
collections (their min and max beside it).  Every shape is a GPU step of its own: a child process under its own time limit; the parent
never opens the device and stops at the first step that fails.  Every yardstick is existing code, timed in the same process:
  (a) k_hsb (sl_hsb_augment) to uint8 beside k_hed (sl_hed_augment) and k_apply (sl_normalize_apply) on the same tiles: all three move
      6 B/px, each with its achieved TB/s
  (b) sl_normalize_hsb_view beside sl_normalize_view (k_view, the jitter route) and sl_normalize_hed_view on the same windows
  (c) end to end, fits included: augment_batch(hsb=, view=, tensor_format=) against the chain augment_batch -> HsbColorAugmenter.
      transform_batch(view=, tensor_format=) with the same draws and windows
The chain's result equals the fused call's bit for bit (checked once per shape before timing)."""
import argparse
import statistics
import subprocess
import sys
import time


def step(shape, collections):
    sys.path.insert(0, ".")
    import numpy as np
    import torch
    import stainlib_amd
    from stainlib_amd import engine
    from stainlib_amd.augmentation.hsb import hsb_codes
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

    def row(label, t, bytes_moved=None):
        tail = "   %.2f TB/s" % (bytes_moved / (t[0] * 1e-3) / 1e12) if bytes_moved else ""
        return "  %-92s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    aug = stainlib_amd.HsbLightColorAugmenter()
    hed = stainlib_amd.HedLighterColorAugmenter()
    rgb = synth_tiles(n, size, size, seed=9)
    dev = rgb.device
    px = n * size * size
    M, maxC, status = engine.macenko_fit(rgb)
    assert int((status != 0).sum()) == 0
    Mt, ct = nz._target_on(dev)
    np.random.seed(3)
    ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=dev)
    hsig, hbia = (torch.as_tensor(x, device=dev) for x in hed.randomize_batch(n))
    sig = aug.randomize_batch(n)
    codes = torch.from_numpy(hsb_codes(sig)).to(dev)
    view = stainlib_amd.TileView(crop)
    win = view.draw(n, size, size)
    dwin = torch.from_numpy(win).to(dev)
    u8 = torch.empty_like(rgb)
    tv = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
    th = torch.empty_like(tv)
    ws = engine.Workspace()
    hws = engine.Workspace()
    route = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct, alpha_beta=ab)
    applied = torch.ones((n,), dtype=torch.int32, device=dev)

    def chain():
        x = nz.augment_batch(rgb, ab, out=u8, ws=ws)[0]
        return aug.transform_batch(x, sig, out=tv, tensor_format=f16, view=view, windows=dwin)[0]

    def fused():
        return nz.augment_batch(rgb, ab, out=th, ws=ws, tensor_format=f16, view=view, windows=dwin, hsb=aug, hsb_sigmas=sig)[0]

    assert torch.equal(chain(), fused()), "the chain and the fused call disagree"
    lines = ["", "%d tiles of %d^2 -> %d^2, float16 NCHW (%.1f Mpx read, %.1f written), codes %s" % (
        n, size, crop, px / 1e6, n * crop * crop / 1e6, sorted(set(win[:, 2].tolist())))]
    ta = timed(lambda: engine.normalize_apply(rgb, M, maxC, Mt, ct, out=u8))
    te = timed(lambda: engine.hed_augment(rgb, hsig, hbia, out=u8, ws=hws))
    tb = timed(lambda: engine.hsb_augment(rgb, codes, out=u8))
    lines.append(row("(a) k_apply (sl_normalize_apply), 3 B/px read + 3 written", ta, 6 * px))
    lines.append(row("    k_hed + its fix-up (sl_hed_augment), 3 B/px read + 3 written", te, 6 * px))
    lines.append(row("    k_hsb (sl_hsb_augment) to uint8, 3 B/px read + 3 written", tb, 6 * px))
    lines.append("    k_hsb takes %.2f of k_apply's time and %.2f of sl_hed_augment's" % (tb[0] / ta[0], tb[0] / te[0]))
    tk = timed(lambda: engine.normalize_view(rgb, dwin, crop, 7, fmt=f16, out=tv, **route))
    thv = timed(lambda: engine.normalize_hed_view(rgb, dwin, crop, 7, hsig, hbia, applied, 0, fmt=f16, out=th, **route))
    tbv = timed(lambda: engine.normalize_hsb_view(rgb, dwin, crop, 7, codes, fmt=f16, out=th, **route))
    lines.append(row("(b) sl_normalize_view (k_view, jitter route) -> float16 NCHW", tk))
    lines.append(row("    sl_normalize_hed_view on the same windows", thv))
    lines.append(row("    sl_normalize_hsb_view on the same windows", tbv))
    lines.append("    the HSB stage takes the view pass to %.2f of its time (the HED stage: %.2f)" % (tbv[0] / tk[0], thv[0] / tk[0]))
    tc, tf = timed(chain), timed(fused)
    lines.append(row("(c) chain with the fit: augment_batch -> HsbColorAugmenter.transform_batch(view=, tensor_format=)", tc))
    lines.append(row("    fused with the fit: augment_batch(hsb=, view=, tensor_format=)", tf))
    lines.append("    the fused call takes %.2f of the chain's time" % (tf[0] / tc[0]))
    print("device %s" % torch.cuda.get_device_name(0))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hsb_time.txt")
    ap.add_argument("--shapes", default="512x1024:896,1250x512:448")
    ap.add_argument("--collections", type=int, default=5)
    ap.add_argument("--step", help="(internal) one shape, in this process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per shape")
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.collections)
    head, body = None, []
    for shape in args.shapes.split(","):                      # one GPU step per shape, each under its own time limit; stop at a failure
        r = subprocess.run([sys.executable, __file__, "--step", shape, "--collections", str(args.collections)], capture_output=True,
                           text=True, timeout=args.step_timeout)
        if r.returncode != 0:
            sys.exit("shape %s failed (exit status %d):\n%s" % (shape, r.returncode, (r.stdout + r.stderr)[-3000:]))
        dev, _, rest = r.stdout.partition("\n")
        head = head or dev
        body.append(rest.rstrip("\n"))
    text = "%s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up\n%s\n" % (
        head, args.collections, "\n".join(body))
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
