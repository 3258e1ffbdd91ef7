"""Pooled slide-level Reinhard (csrc/slide_lab.hip) beside the per-tile ReinhardStainNormalizer.transform_batch on the same
device-resident tiles.
    python tools/pooled_reinhard_time.py [--out profiles/pooled_reinhard_scale.txt]
Two slides in one process: 1 250 tiles of 512^2 and 512 tiles of 1024^2.  For each, by HIP events after a spin-up, three repetitions of
the per-tile transform_batch and three of the pooled SlideNormalizer.transform_shard (its read-back included), then the pooled mode's
three sweeps one by one with their fraction of 8 TB/s at 4, 4 and 6 B/px (the bytes a dwordx3-chunked sweep moves per pixel are 3, 3
and 6; both are printed).  The condition the file states: the pooled median is not slower than the per-tile median by more than the
spread (max - min) of the three per-tile repetitions of the same run."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import stainlib_amd as sl  # noqa: E402
from stainlib_amd import engine  # noqa: E402
from stainlib_amd.distributed import SlideNormalizer  # noqa: E402
from tools.synth import synth_tiles  # noqa: E402

PEAK = 8.0e12          # B/s


def timed(fn, reps):
    """ms per call: spin-up (the clocks ramp for ~25 ms), then `reps` calls between two events"""
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.25:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pooled_reinhard_scale.txt")
    ap.add_argument("--shapes", default="1250x512,512x1024")
    args = ap.parse_args()
    nrm = sl.ReinhardStainNormalizer()
    st = engine.reinhard_stats(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]]), standardize=True)[0].cpu().numpy()
    nrm.target_means, nrm.target_stds = tuple(st[1:4]), tuple(st[4:7])
    tm, ts = nrm._targets()
    lines = ["pooled slide-level Reinhard vs per-tile transform_batch, ms per slide (HIP events after a 0.25 s spin-up), device %s"
             % torch.cuda.get_device_name(0)]
    for shape in args.shapes.split(","):
        n, size = (int(x) for x in shape.split("x"))
        rgb = synth_tiles(n, size, size, seed=9)
        out = torch.empty_like(rgb)
        ws = engine.Workspace()
        pooled = SlideNormalizer(nrm, group=False, mode="pooled")
        reps = 5
        per_tile_ms = [timed(lambda: nrm.transform_batch(rgb, out=out, ws=ws), reps) for _ in range(3)]
        pooled_ms = [timed(lambda: pooled.transform_shard(rgb, out=out), reps) for _ in range(3)]
        med_t, med_p = statistics.median(per_tile_ms), statistics.median(pooled_ms)
        spread = max(per_tile_ms) - min(per_tile_ms)
        px = n * size * size
        lines.append("")
        lines.append("%d tiles of %d^2 (%.1f Mpx)" % (n, size, px / 1e6))
        lines.append("  per-tile transform_batch   %s   median %.3f  spread %.3f" % ("  ".join("%.3f" % v for v in per_tile_ms), med_t, spread))
        lines.append("  pooled transform_shard     %s   median %.3f  (p90 %.1f)" % ("  ".join("%.3f" % v for v in pooled_ms), med_p, pooled.last_p90))
        ok = med_p <= med_t + spread
        lines.append("  pooled / per-tile = %.3f : %s" % (med_p / med_t, "pooled is not slower than per-tile by more than the per-tile spread"
                                                          if ok else "POOLED IS SLOWER than per-tile by more than the per-tile spread"))
        # the three sweeps of the pooled chain, one by one (the state of a finished chain: the tables the sweeps read)
        wsl = engine.slab_workspace(n, size, size, rgb.device)
        state = engine.slab_begin(engine.slab_bytes(rgb, wsl), True, rgb.device)
        engine.slab_finish(state, engine.slab_lab(rgb, state, 0.8, wsl), 0, tm, ts)
        sa = torch.empty((256,), dtype=torch.int64, device=rgb.device)
        sb = torch.empty((262,), dtype=torch.int64, device=rgb.device)
        sweeps = (("sl_slab_bytes", lambda: engine.slab_bytes(rgb, wsl, sums=sa), 4, 3),
                  ("sl_slab_lab", lambda: engine.slab_lab(rgb, state, 0.8, wsl, sums=sb), 4, 3),
                  ("sl_slab_map", lambda: engine.slab_map(rgb, state, 0, out=out), 6, 6))
        total = 0.0
        for name, fn, nominal, moved in sweeps:
            ms = timed(fn, reps)
            total += ms
            lines.append("  %-14s %.3f ms   %.2f of 8 TB/s at %d B/px   (%.2f at the %d B/px it moves)"
                         % (name, ms, px * nominal / (ms * 1e-3) / PEAK, nominal, px * moved / (ms * 1e-3) / PEAK, moved))
        lines.append("  sweeps together %.3f ms; the rest of the chain (two reduce kernels, two steps, the read-back) %.3f ms" % (total, med_p - total))
        del rgb, out
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
