"""What the post stage -- the tone curve and the additive noise on the bytes a call writes -- costs, beside its yardsticks and beside the
torch chain a loader runs behind the call without it.
    python tools/post_time.py [--out profiles/post_time.txt] [--shapes 512x1024:896] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko).  Per shape (n tiles of size^2 -> crop^2, float16 NCHW, jitter route), timed by HIP
events after a 0.25 s spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median
of the collections (their min and max beside it).  Every shape is a GPU step of its own: a child process under its own time limit; the
parent never opens the device and stops at the first step that fails.  Every yardstick is existing code, timed in the same process:
  (a) k_post (sl_post_augment) to uint8 -- noise only, tone only, both -- beside k_apply (sl_normalize_apply) and k_hsb (sl_hsb_augment)
      on the same bytes: all move 6 B/px, each with its achieved TB/s
  (b) sl_normalize_post_view beside sl_normalize_view (k_view, the jitter route) on the same windows, at shrink 1 and 2
  (c) end to end, fits included: augment_batch(noise=, tone=, view=, tensor_format=) against augment_batch(view=, tensor_format=)
      followed by torch on the float16 tensor: x ** gamma, * contrast + offset, + sigma * randn_like, clamp.  That chain is the work the
      stage replaces and ANOTHER definition (a float curve, torch's generator), not a reference for bits.
The fused call equals post_reference of the plain view bit for bit (checked once per shape, on the first tiles, before timing)."""
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
    from stainlib_amd.augmentation.noise import post_reference
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
        return "  %-100s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16)
    noise = stainlib_amd.GaussianNoiseAugmenter((2, 10))
    tone = stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), (0.8, 1.25), (0.7, 1.4))
    hsb = stainlib_amd.HsbLightColorAugmenter()
    rgb = synth_tiles(n, size, size, seed=9)
    dev = rgb.device
    px = n * size * size
    M, maxC, status = engine.macenko_fit(rgb)
    assert int((status != 0).sum()) == 0
    Mt, ct = nz._target_on(dev)
    np.random.seed(3)
    ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=dev)
    hcodes = torch.from_numpy(hsb_codes(hsb.randomize_batch(n))).to(dev)
    params, tables_h = tone.randomize_batch(n)
    sigmas, codes_h = noise.randomize_batch(n)
    tables, codes = torch.from_numpy(tables_h).to(dev), torch.from_numpy(codes_h).to(dev)
    view = stainlib_amd.TileView(crop)
    win = view.draw(n, size, size)
    dwin = torch.from_numpy(win).to(dev)
    view2 = stainlib_amd.TileView(crop // 2, shrink=2)
    dwin2 = torch.from_numpy(view2.draw(n, size, size)).to(dev)
    u8 = torch.empty_like(rgb)
    tv = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
    th = torch.empty_like(tv)
    tv2 = torch.empty((n, 3, crop // 2, crop // 2), dtype=torch.float16, device=dev)
    ws = engine.Workspace()
    route = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct, alpha_beta=ab)
    # the torch chain's per-tile constants, on the [0, 1] scale of the tensor
    tp = torch.as_tensor(params, device=dev, dtype=torch.float16)
    gam, con = tp[:, 2].view(n, 1, 1, 1), tp[:, 1].view(n, 1, 1, 1)
    off = (0.5 - 0.5 * tp[:, 1] + tp[:, 0]).view(n, 1, 1, 1)
    sig = torch.as_tensor(sigmas / 255.0, device=dev, dtype=torch.float16).view(n, 1, 1, 1)

    def chain():
        x = nz.augment_batch(rgb, ab, out=tv, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]
        x = torch.pow(x, gam) * con + off
        x = x + sig * torch.randn_like(x)
        return x.clamp_(0.0, 1.0)

    def fused():
        return nz.augment_batch(rgb, ab, out=th, ws=ws, tensor_format=f16, view=view, windows=dwin, noise=noise, tone=tone,
                                noise_sigmas=codes, tone_params=tables)[0]

    k = min(n, 2)                                               # the definition, on the first tiles
    plain = nz.augment_batch(rgb[:k], ab[:k], view=view, windows=dwin[:k])[0]
    want = torch.from_numpy(post_reference(plain.cpu().numpy(), tables=tables_h[:k], codes=codes_h[:k])).to(dev)
    assert torch.equal(fused()[:k], f16.convert(want)), "the fused call is not post_reference of the plain view"
    lines = ["", "%d tiles of %d^2 -> %d^2, float16 NCHW (%.1f Mpx read, %.1f written), codes %s" % (
        n, size, crop, px / 1e6, n * crop * crop / 1e6, sorted(set(win[:, 2].tolist())))]
    ta = timed(lambda: engine.normalize_apply(rgb, M, maxC, Mt, ct, out=u8))
    tb = timed(lambda: engine.hsb_augment(rgb, hcodes, out=u8))
    tn = timed(lambda: engine.post_augment(rgb, codes=codes, out=u8))
    tt = timed(lambda: engine.post_augment(rgb, tables=tables, out=u8))
    t2 = timed(lambda: engine.post_augment(rgb, tables=tables, codes=codes, out=u8))
    lines.append(row("(a) k_apply (sl_normalize_apply), 3 B/px read + 3 written", ta, 6 * px))
    lines.append(row("    k_hsb (sl_hsb_augment) to uint8, 3 B/px read + 3 written", tb, 6 * px))
    lines.append(row("    k_post (sl_post_augment) to uint8, noise only", tn, 6 * px))
    lines.append(row("    k_post (sl_post_augment) to uint8, tone only", tt, 6 * px))
    lines.append(row("    k_post (sl_post_augment) to uint8, tone and noise", t2, 6 * px))
    lines.append("    k_post takes %.2f (noise) / %.2f (tone) / %.2f (both) of k_apply's time and %.2f / %.2f / %.2f of k_hsb's" % (
        tn[0] / ta[0], tt[0] / ta[0], t2[0] / ta[0], tn[0] / tb[0], tt[0] / tb[0], t2[0] / tb[0]))
    tk = timed(lambda: engine.normalize_view(rgb, dwin, crop, 7, fmt=f16, out=tv, **route))
    tpv = timed(lambda: engine.normalize_post_view(rgb, dwin, crop, 7, tables=tables, codes=codes, fmt=f16, out=th, **route))
    tpn = timed(lambda: engine.normalize_post_view(rgb, dwin, crop, 7, codes=codes, fmt=f16, out=th, **route))
    tpt = timed(lambda: engine.normalize_post_view(rgb, dwin, crop, 7, tables=tables, fmt=f16, out=th, **route))
    tk2 = timed(lambda: engine.normalize_view(rgb, dwin2, crop // 2, 7, fmt=f16, out=tv2, shrink=2, **route))
    tp2 = timed(lambda: engine.normalize_post_view(rgb, dwin2, crop // 2, 7, tables=tables, codes=codes, fmt=f16, out=tv2, shrink=2, **route))
    lines.append(row("(b) sl_normalize_view (k_view, jitter route) -> float16 NCHW, shrink 1", tk))
    lines.append(row("    sl_normalize_post_view on the same windows, tone and noise", tpv))
    lines.append(row("    sl_normalize_post_view on the same windows, noise only", tpn))
    lines.append(row("    sl_normalize_post_view on the same windows, tone only", tpt))
    lines.append(row("    sl_normalize_view, shrink 2 (%d^2 windows -> %d^2)" % (crop, crop // 2), tk2))
    lines.append(row("    sl_normalize_post_view on the same windows, shrink 2, tone and noise", tp2))
    lines.append("    the post stage takes the view pass to %.2f of its time at shrink 1 (noise only %.2f, tone only %.2f) and to %.2f at shrink 2"
                 % (tpv[0] / tk[0], tpn[0] / tk[0], tpt[0] / tk[0], tp2[0] / tk2[0]))
    tc, tf = timed(chain), timed(fused)
    lines.append(row("(c) chain with the fit: augment_batch(view=, tensor_format=) -> torch pow, * a + b, + sigma * randn_like, clamp", tc))
    lines.append(row("    fused with the fit: augment_batch(noise=, tone=, view=, tensor_format=)", tf))
    lines.append("    the fused call takes %.2f of the chain's time" % (tf[0] / tc[0]))
    print("device %s" % torch.cuda.get_device_name(0))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/post_time.txt")
    ap.add_argument("--shapes", default="512x1024:896")
    ap.add_argument("--collections", type=int, default=5)
    ap.add_argument("--step", help="(internal) one shape, in this process")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per shape")
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
