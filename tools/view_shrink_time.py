"""What the 2x / 4x box shrink inside the view passes costs, beside the unshrunk view of the same window and beside the chain it replaces,
view -> torch.nn.functional.avg_pool2d.
    python tools/view_shrink_time.py [--out profiles/view_shrink_time.txt] [--tiles 512] [--size 1024] [--collections 5]
Device-resident synthetic tiles.  512 tiles of 1024^2 -> 448^2 at s = 2 and -> 224^2 at s = 4 (an 896^2 window either way), float16 NCHW,
mixed codes and corners from TileView.draw.  Timed by HIP events after a 0.25 s spin-up of the same call; a COLLECTION is the median of 20
single launches, and the figure in the file is the median of the collections (their min and max beside it).  Every yardstick is existing
code, timed in the same process as what it is compared with:
  (a) sl_normalize_view_shrink (the jitter route) beside sl_normalize_view on the same source windows at s = 1: the same reads and the same
      per-source-pixel arithmetic, so the difference is the write side alone (s s LDS reads per output pixel, 1 / s s of the stores)
  (b) end to end, fits included: augment_batch(view=shrunk, tensor_format=f) against augment_batch(view=window at s size, tensor_format=f)
      -> avg_pool2d(., s)
  (c) the same pair for ReinhardStainNormalizer.transform_batch(mask_background=True)
  (d) sl_normalize_view at s = 1 on the shapes of tools/view_time.py (512 x 1024^2 -> 896^2, 4096 x 256^2 -> 224^2; jitter route, float16
      NCHW): the figure to put beside an earlier build's
(The chain of (b) and (c) averages float16 values and rounds once more; the fused pass averages bytes.  They are different definitions
and are not compared bit for bit; the largest difference is printed.)
Each step runs in a process of its own under `timeout`; a step that ends with a non-zero status ends the run, and nothing further is
started on the device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

STEPS = ("a", "b", "c", "d")


def step(args):
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
        ms = [collection(fn) for _ in range(args.collections)]
        return statistics.median(ms), min(ms), max(ms)

    def row(label, t):
        return "  %-100s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])

    target = synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy()
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    n, size = args.tiles, args.size
    window = size // 128 * 112                                  # 896 out of 1024: the window both shrinks take
    lines = []

    def jitter_setup(n, size):
        nz = stainlib_amd.MacenkoNormalizer()
        nz.fit(target)
        rgb = synth_tiles(n, size, size, seed=9)
        M, maxC, status = engine.macenko_fit(rgb)
        assert int((status != 0).sum()) == 0
        Mt, ct = nz._target_on(rgb.device)
        np.random.seed(3)
        ab = torch.as_tensor(stainlib_amd.StainJitter().draw(n), device=rgb.device)
        return nz, rgb, (M, maxC, Mt, ct, ab)

    def windows(n, size, crop):
        np.random.seed(4)
        win = stainlib_amd.TileView(crop).draw(n, size, size)
        return win, torch.from_numpy(win).cuda()

    if args.step == "a":
        nz, rgb, route = jitter_setup(n, size)
        win, dwin = windows(n, size, window)
        full = torch.empty((n, 3, window, window), dtype=torch.float16, device=rgb.device)
        t1 = timed(lambda: engine.normalize_view(rgb, dwin, window, 7, *route, fmt=f16, out=full))
        lines.append("(a) %d tiles of %d^2, %d^2 windows, jitter route -> float16 NCHW, codes %s" % (n, size, window, sorted(set(win[:, 2].tolist()))))
        lines.append(row("sl_normalize_view, s = 1 -> %d^2 (6 B written per source px)" % window, t1))
        for s in (2, 4):
            out = torch.empty((n, 3, window // s, window // s), dtype=torch.float16, device=rgb.device)
            ts = timed(lambda: engine.normalize_view(rgb, dwin, window // s, 7, *route, fmt=f16, out=out, shrink=s))
            lines.append(row("sl_normalize_view_shrink, s = %d -> %d^2 (%.3f B written per source px)" % (s, window // s, 6.0 / (s * s)), ts))
            lines.append("    s = %d takes %.2f of the unshrunk view's time" % (s, ts[0] / t1[0]))
    elif args.step in ("b", "c"):
        if args.step == "b":
            nz, rgb, route = jitter_setup(n, size)
            ab = route[4]
            ws = engine.Workspace()
            call = lambda view, dwin, out: nz.augment_batch(rgb, ab, out=out, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]      # noqa: E731
            what = "augment_batch"
        else:
            nz = stainlib_amd.ReinhardStainNormalizer()
            nz.fit(target)
            rgb = synth_tiles(n, size, size, seed=9)
            ws = engine.Workspace()
            call = lambda view, dwin, out: nz.transform_batch(rgb, mask_background=True, out=out, ws=ws, tensor_format=f16, view=view,   # noqa: E731
                                                              windows=dwin)[0]
            what = "ReinhardStainNormalizer.transform_batch"
        win, dwin = windows(n, size, window)
        full = torch.empty((n, 3, window, window), dtype=torch.float16, device=rgb.device)
        big = stainlib_amd.TileView(window)
        lines.append("(%s) %s, fits / statistics included; %d tiles of %d^2, %d^2 windows -> float16 NCHW" % (args.step, what, n, size, window))
        for s in (2, 4):
            small = stainlib_amd.TileView(window // s, shrink=s)
            out = torch.empty((n, 3, window // s, window // s), dtype=torch.float16, device=rgb.device)
            chain = lambda: torch.nn.functional.avg_pool2d(call(big, dwin, full), s)                                                      # noqa: E731
            fused = lambda: call(small, dwin, out)                                                                                        # noqa: E731
            diff = float((chain().float() - fused().float()).abs().max())
            tc, tf = timed(chain), timed(fused)
            lines.append(row("chain: %s(view=%d^2, tensor_format=) -> avg_pool2d(%d)" % (what, window, s), tc))
            lines.append(row("fused: %s(view=%d^2 at shrink=%d, tensor_format=)" % (what, window // s, s), tf))
            lines.append("    s = %d: the fused call takes %.2f of the chain's time%s; largest |chain - fused| = %.4f (different roundings)" % (
                s, tf[0] / tc[0], "" if tf[0] < tc[0] else "  -- the fused pass is not faster at this shape", diff))
    else:
        lines.append("(d) sl_normalize_view at s = 1 (jitter route -> float16 NCHW) on the shapes of tools/view_time.py")
        for n2, size2, crop in ((512, 1024, 896), (4096, 256, 224)):
            nz, rgb, route = jitter_setup(n2, size2)
            win, dwin = windows(n2, size2, crop)
            out = torch.empty((n2, 3, crop, crop), dtype=torch.float16, device=rgb.device)
            lines.append(row("sl_normalize_view %d x %d^2 -> %d^2" % (n2, size2, crop),
                             timed(lambda: engine.normalize_view(rgb, dwin, crop, 7, *route, fmt=f16, out=out))))
            del rgb, out, nz, route
            torch.cuda.empty_cache()
    head = "device %s; " % torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        f.write(head + "\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/view_shrink_time.txt")
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--collections", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each step's process may take")
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process and write its lines to --part")
    ap.add_argument("--part")
    args = ap.parse_args()
    if args.step:
        return step(args)
    text = ["ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up; one process per "
            "step" % args.collections]
    rc = 0
    for name in STEPS:
        part = "%s.%s.part" % (args.out, name)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--part", part,
               "--tiles", str(args.tiles), "--size", str(args.size), "--collections", str(args.collections)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                               # a fault, an abort or the time limit: nothing further on the device
            text += ["", "(%s) ended with status %d: not measured, and the steps behind it were not started" % (name, rc)]
            break
        body = open(part).read().splitlines()
        os.remove(part)
        if len(text) == 1:
            text[0] = body[0] + text[0]
        text += [""] + body[1:]
    out = "\n".join(text) + "\n"
    print(out, flush=True)
    with open(args.out, "w") as f:
        f.write(out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
