"""What the one-pass recipe -- a colour stage on source pixels, an affine or elastic view and tone / noise on written pixels in ONE launch --
costs, beside the view alone and beside the shortest chain of existing calls that gives the same bits.
    python tools/recipe_time.py [--out profiles/recipe_time.txt] [--shapes 512x1024:896] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko).  Per shape (n tiles of size^2 -> crop^2, float16 NCHW, jitter route), timed by HIP
events after a 0.25 s spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median
of the collections (their min and max beside it).  Every shape is a GPU step of its own: a child process under its own time limit; the
parent never opens the device and stops at the first step that fails.  Every yardstick is existing code, timed in the same process:
  (a) sl_normalize_stages_view_elastic with HSB, with noise, with both (and with tone beside them), beside sl_normalize_view_elastic on the
      same rows and field; the same for sl_normalize_stages_view_affine beside sl_normalize_view_affine
  (b) end to end, fits included: augment_batch(recipe=Recipe(TileElastic, Hsb, noise, tone), tensor_format=) against the shortest chain of
      existing calls with the same bits: augment_batch(hsb=) to the full uint8 tile -> convert(view=elastic) to uint8 ->
      noise.transform_batch(codes, tensor_format=) behind tone.transform_batch(tables)
There is no pass mark.  The fused call equals the chain bit for bit (checked once per shape, on the first tiles, before timing)."""
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

    def row(label, t, base=None):
        tail = "   %.2f of the view alone" % (t[0] / base[0]) if base else ""
        return "  %-100s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16)
    noise = stainlib_amd.GaussianNoiseAugmenter((2, 10))
    tone = stainlib_amd.ToneCurveAugmenter((-0.1, 0.1), (0.8, 1.25), (0.7, 1.4))
    hsb = stainlib_amd.HsbLightColorAugmenter()
    view = stainlib_amd.TileElastic(crop, rotate=(-180, 180), zoom=(0.9, 1.1), magnitude=(1, 4), cell=32)
    recipe = stainlib_amd.Recipe(view, hsb, noise, tone)
    rgb = synth_tiles(n, size, size, seed=9)
    dev = rgb.device
    M, maxC, status = engine.macenko_fit(rgb)
    assert int((status != 0).sum()) == 0
    Mt, ct = nz._target_on(dev)
    np.random.seed(3)
    ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=dev)
    hs = np.array(hsb.randomize_batch(n), dtype=np.float64)
    hcodes = torch.from_numpy(hsb_codes(hs)).to(dev)
    params, tables_h = tone.randomize_batch(n)
    sigmas, codes_h = noise.randomize_batch(n)
    tables, codes = torch.from_numpy(tables_h).to(dev), torch.from_numpy(codes_h).to(dev)
    win = view.draw(n, size, size)
    rows, field = torch.from_numpy(win.affine).to(dev), torch.from_numpy(win.field).to(dev)
    dwin = stainlib_amd.ElasticWindows(rows, field)
    max_r, max_d = view.bound, view.max_d
    tv = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
    th = torch.empty_like(tv)
    u8 = torch.empty_like(rgb)
    v8 = torch.empty((n, crop, crop, 3), dtype=torch.uint8, device=dev)
    t8 = torch.empty_like(v8)
    ws = engine.Workspace()
    route = dict(M_src=M, maxC_src=maxC, M_tgt=Mt, maxC_tgt=ct, alpha_beta=ab)
    draw = engine.RecipeDraw(dwin, engine.HsbDraw(hs, hcodes), engine.PostDraw(params, tables, sigmas, codes))

    def chain():
        full = nz.augment_batch(rgb, ab, out=u8, ws=ws, hsb=hsb, hsb_sigmas=hs)[0]
        cut = engine.view_pass(full, view, dwin, out=v8)[0]
        toned = tone.transform_batch(cut, tables, out=t8)[0]
        return noise.transform_batch(toned, codes, out=tv, tensor_format=f16)[0]

    def fused():
        return nz.augment_batch(rgb, ab, out=th, ws=ws, tensor_format=f16, recipe=recipe, recipe_draw=draw)[0]

    k = min(n, 2)                                               # the same bits, on the first tiles
    a, b = chain(), fused()
    assert torch.equal(a[:k].view(torch.int16), b[:k].view(torch.int16)), "the fused call is not the chain"
    lines = ["", "%d tiles of %d^2 -> %d^2, float16 NCHW (%.1f Mpx read, %.1f written), max_r %d / 65536, max_d %d, cell %d" % (
        n, size, crop, n * size * size / 1e6, n * crop * crop / 1e6, max_r, max_d, view.cell)]
    stage_sets = (("HSB", dict(hsb_codes=hcodes)), ("noise", dict(codes=codes)), ("tone", dict(tables=tables)),
                  ("HSB and noise", dict(hsb_codes=hcodes, codes=codes)), ("HSB, tone and noise", dict(hsb_codes=hcodes, tables=tables, codes=codes)))
    te = timed(lambda: engine.normalize_view_elastic(rgb, rows, field, crop, view.cell, max_r, max_d, fmt=f16, out=tv, **route))
    lines.append(row("(a) sl_normalize_view_elastic (jitter route) -> float16 NCHW", te))
    for name, st in stage_sets:
        t = timed(lambda: engine.normalize_stages_view_elastic(rgb, rows, field, crop, view.cell, max_r, max_d, fmt=f16, out=th, **route, **st))
        lines.append(row("    sl_normalize_stages_view_elastic on the same rows and field, %s" % name, t, te))
    ta = timed(lambda: engine.normalize_view_affine(rgb, rows, crop, max_r, fmt=f16, out=tv, **route))
    lines.append(row("    sl_normalize_view_affine (jitter route) on the same rows -> float16 NCHW", ta))
    for name, st in stage_sets:
        t = timed(lambda: engine.normalize_stages_view_affine(rgb, rows, crop, max_r, fmt=f16, out=th, **route, **st))
        lines.append(row("    sl_normalize_stages_view_affine on the same rows, %s" % name, t, ta))
    tc, tf = timed(chain), timed(fused)
    lines.append(row("(b) chain with the fit: augment_batch(hsb=) -> view_pass(elastic) to uint8 -> tone.transform_batch -> noise.transform_batch(f16)", tc))
    lines.append(row("    fused with the fit: augment_batch(recipe=Recipe(TileElastic, Hsb, noise, tone), tensor_format=)", tf))
    lines.append("    the fused call takes %.2f of the chain's time" % (tf[0] / tc[0]))
    print("device %s" % torch.cuda.get_device_name(0))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/recipe_time.txt")
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
