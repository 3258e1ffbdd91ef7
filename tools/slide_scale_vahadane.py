"""Pooled slide-level Vahadane (csrc/slide_dict.hip) beside median-mode Vahadane and per-tile vahadane_transform, on the same
device-resident 1024^2 tiles (development aid).
    python tools/slide_scale_vahadane.py [n,n,...]      (default 512,12500 tiles of 1024^2 = up to 39 GB in + 39 GB out)
One JSON line per (slide size, path): ms per slide after a spin-up, tiles/s, and for the pooled path the dictionary rounds, the full
sweeps among them and how the concentration stage settled ("window": one sweep, "radix": the fallback rounds)."""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import stainlib_amd as sl  # noqa: E402
from stainlib_amd import engine  # noqa: E402
from stainlib_amd.distributed import SlideNormalizer  # noqa: E402
from tools.synth import synth_tiles  # noqa: E402

sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [512, 12500]
tgt = synth_tiles(1, 1024, 1024, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])
Mt, mct, _, _ = engine.vahadane_fit(tgt)
nrm = sl.VahadaneNormalizer()
nrm.stain_matrix_target, nrm.maxC_target = Mt[0].cpu().numpy(), mct[0].cpu().numpy().reshape(1, 2)
Mt_d, mct_d = Mt[0].contiguous(), mct[0].contiguous()
nmax = max(sizes)
rgb_all = synth_tiles(nmax, 1024, 1024, seed=9)
out_all = torch.empty_like(rgb_all)
ws = engine.Workspace()
for n in sizes:
    rgb, out = rgb_all[:n], out_all[:n]
    pooled = SlideNormalizer(nrm, group=False, mode="pooled")
    median = SlideNormalizer(nrm, group=False, mode="median")
    runs = {"pooled": lambda: pooled.transform_shard(rgb, out=out),
            "median": lambda: median.transform_shard(rgb, out=out),
            "per_tile": lambda: engine.vahadane_transform(rgb, Mt_d, mct_d, out=out, ws=ws)}
    for name, fn in runs.items():
        t_spin = time.perf_counter()
        while time.perf_counter() - t_spin < 0.25:           # spin-up: the clocks ramp for ~25 ms
            fn()
        torch.cuda.synchronize()
        reps = 10 if n <= 512 else 2
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / reps * 1e3
        line = {"tiles": n, "size": 1024, "path": name, "ms": round(ms, 3), "tiles_per_s": round(n / ms * 1e3, 1)}
        if name == "pooled":
            line.update(rounds=pooled.last_rounds, full_sweeps=pooled.last_sweeps, maxc_path=pooled.last_path)
        print(json.dumps(line), flush=True)
