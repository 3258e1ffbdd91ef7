"""What the stain separation inside the view pass costs, beside the full-tile separation and beside the chain it replaces
(DESIGN.md 4.18).
    python tools/separate_view_time.py [--out profiles/separate_view_time.txt] [--collections 5]
Device-resident synthetic tiles, mixed codes and corners from TileView.draw.  Timed by HIP events after a 0.25 s spin-up of the same call; a
COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections (their min and max beside it).
Every yardstick is existing code, timed in the same process as what it is compared with:
  (a) sl_stain_separate_view, all four outputs (uint8 images, float32 planes), 4096 x 256^2 -> 224^2 and 512 x 1024^2 -> 896^2, beside
      sl_stain_separate on the full tiles of the same batch: times, and bytes written per second (17 B per written pixel either way)
  (b) end to end, fits included: separate_batch(want=("h", "conc"), conc_dtype=float16, tensor_format=f16, view=) against the chain
      separate_batch(want=("h", "conc"), conc_dtype=float16) -> tensor_format.convert -> torch slice / flip / rot90 per tile on the same
      windows (512 x 1024^2 -> 896^2)
  (c) shrink = 2, images only: separate_batch(want=("h", "e"), tensor_format=f16, view=TileView(448, shrink=2)) against the chain
      separate_batch -> convert -> slice / flip / rot90 -> avg_pool2d(2).  (The chain averages float16 values and rounds once more; the
      fused pass averages bytes.  They are different definitions and are not compared bit for bit; the largest difference is printed.)
Each step runs in a process of its own under `timeout`; a step that ends with a non-zero status ends the run, and nothing further is
started on the device."""
import argparse
import os
import statistics
import subprocess
import sys
import time

STEPS = ("a", "b", "c")


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

    def row(label, t, tail=""):
        return "  %-104s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    target = synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy()
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    lines = []

    def setup(n, size):
        nz = stainlib_amd.MacenkoNormalizer()
        nz.fit(target)
        rgb = synth_tiles(n, size, size, seed=9)
        M, maxC, status = engine.macenko_fit(rgb)
        assert int((status != 0).sum()) == 0
        Mt, ct = nz._target_on(rgb.device)
        return nz, rgb, (M, maxC, Mt, ct)

    def windows(n, size, view):
        np.random.seed(4)
        win = view.draw(n, size, size)
        return win, torch.from_numpy(win).cuda()

    def torch_view(x, win, oh, ow, out, s=1):
        """the chain's last step: per tile the window of the (N, C, H, W) tensor x, flipped and turned (and pooled), into out"""
        for t, (y0, x0, d) in enumerate(win.tolist()):
            wh, ww = (ow, oh) if d & 1 else (oh, ow)
            v = x[t, :, y0:y0 + s * wh, x0:x0 + s * ww]
            if d & 4:
                v = torch.flip(v, dims=(2,))
            v = torch.rot90(v, d & 3, dims=(1, 2))
            out[t] = v if s == 1 else torch.nn.functional.avg_pool2d(v, s)
        return out

    if args.step == "a":
        lines.append("(a) all four outputs: uint8 norm, h, e and float32 conc (17 B written per output pixel)")
        for n, size, crop in ((4096, 256, 224), (512, 1024, 896)):
            nz, rgb, stats = setup(n, size)
            win, dwin = windows(n, size, stainlib_amd.TileView(crop))
            S = engine.Separated
            full = S(*(torch.empty((n, size, size, 3), dtype=torch.uint8, device=rgb.device) for _ in range(3)),
                     torch.empty((n, 2, size, size), dtype=torch.float32, device=rgb.device))
            view = S(*(torch.empty((n, crop, crop, 3), dtype=torch.uint8, device=rgb.device) for _ in range(3)),
                     torch.empty((n, 2, crop, crop), dtype=torch.float32, device=rgb.device))
            tf = timed(lambda: engine.stain_separate(rgb, *stats, out=full))
            tv = timed(lambda: engine.stain_separate_view(rgb, dwin, crop, *stats, out=view))
            gb = lambda px, t: "  %7.1f GB/s written" % (17.0 * px / (t[0] * 1e-3) / 1e9)                                       # noqa: E731
            lines.append(row("sl_stain_separate       %d x %d^2 (full tiles)" % (n, size, ), tf, gb(n * size * size, tf)))
            lines.append(row("sl_stain_separate_view  %d x %d^2 -> %d^2, codes %s" % (n, size, crop, sorted(set(win[:, 2].tolist()))), tv,
                             gb(n * crop * crop, tv)))
            lines.append("    the view takes %.2f of the full-tile call's time for %.2f of its pixels" % (tv[0] / tf[0], (crop / size) ** 2))
            del rgb, full, view, nz, stats
            torch.cuda.empty_cache()
    else:
        n, size, crop = 512, 1024, 896
        nz, rgb, _ = setup(n, size)
        ws = engine.Workspace()
        if args.step == "b":
            view = stainlib_amd.TileView(crop)
            win, dwin = windows(n, size, view)
            out_h = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=rgb.device)
            out_c = torch.empty((n, 2, crop, crop), dtype=torch.float16, device=rgb.device)

            def chain():
                sep = nz.separate_batch(rgb, want=("h", "conc"), conc_dtype=torch.float16, ws=ws)[0]
                return torch_view(f16.convert(sep.h), win, crop, crop, out_h), torch_view(sep.conc, win, crop, crop, out_c)

            def fused():
                sep = nz.separate_batch(rgb, want=("h", "conc"), conc_dtype=torch.float16, ws=ws, tensor_format=f16, view=view, windows=dwin)[0]
                return sep.h, sep.conc

            a, b = chain(), fused()
            same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
            lines.append("(b) separate_batch(want=('h', 'conc'), conc_dtype=float16), fits included; %d tiles of %d^2 -> %d^2, h as float16 NCHW; "
                         "chain and fused agree bit for bit: %s" % (n, size, crop, same))
            what = ("chain: separate_batch -> convert -> torch slice / flip / rot90 per tile", "fused: separate_batch(tensor_format=, view=)")
        else:
            s = 2
            small = crop // s
            view = stainlib_amd.TileView(small, shrink=s)
            win, dwin = windows(n, size, view)
            outs = [torch.empty((n, 3, small, small), dtype=torch.float16, device=rgb.device) for _ in range(2)]

            def chain():
                sep = nz.separate_batch(rgb, want=("h", "e"), ws=ws)[0]
                return [torch_view(f16.convert(x), win, small, small, o, s) for x, o in zip((sep.h, sep.e), outs)]

            def fused():
                sep = nz.separate_batch(rgb, want=("h", "e"), ws=ws, tensor_format=f16, view=view, windows=dwin)[0]
                return [sep.h, sep.e]

            diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(chain(), fused()))
            lines.append("(c) separate_batch(want=('h', 'e')), fits included; %d tiles of %d^2, %d^2 windows -> %d^2 at shrink = %d, float16 NCHW; "
                         "largest |chain - fused| = %.4f (different definitions: the chain averages float16 values, the fused pass bytes)" % (
                             n, size, crop, small, s, diff))
            what = ("chain: separate_batch -> convert -> slice / flip / rot90 -> avg_pool2d(2) per tile",
                    "fused: separate_batch(tensor_format=, view=TileView(%d, shrink=2))" % small)
        tc, tf = timed(chain), timed(fused)
        lines.append(row(what[0], tc))
        lines.append(row(what[1], tf))
        lines.append("    the fused call takes %.2f of the chain's time%s" % (tf[0] / tc[0], "" if tf[0] < tc[0] else
                                                                               "  -- the fused call is not faster at this shape"))
    head = "device %s; " % torch.cuda.get_device_name(0)
    with open(args.part, "w") as f:
        f.write(head + "\n" + "\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/separate_view_time.txt")
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
               "--collections", str(args.collections)]
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
