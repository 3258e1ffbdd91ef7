"""What the crop / flip / rot90 view inside the apply pass costs, beside k_apply_jitter and beside the chain a loader runs without it
(DESIGN.md 4.13).
    python tools/view_time.py [--out profiles/view_time.txt] [--shapes 512x1024:896,4096x256:224] [--collections 5]
Device-resident synthetic tiles, fitted once (Macenko).  Per shape (n tiles of size^2 -> crop^2), timed by HIP events after a 0.25 s
spin-up of the same call; a COLLECTION is the median of 20 single launches, and the figure in the file is the median of the collections
(their min and max beside it).  Tissue-only jitter under a target, mixed codes and corners from TileView.draw; outputs float16 NCHW and
uint8.  Both yardsticks are existing code, timed in the same run:
  1. k_apply_jitter (sl_normalize_jitter) on n tiles of crop^2 -- as many pixels as the view writes -- and sl_normalize_view itself, each
     with its achieved TB/s at 3 B read + the output bytes per written pixel, and the ratio of the two rates
  2. the chain without the view: sl_normalize_jitter on the FULL tiles to the float16 tensor, then torch: per code one gather of the
     windows, flip / rot90, written into the contiguous batch; beside it sl_normalize_view to the same tensor.  Then both with the fit in
     front, as the classes run them: augment_batch(tensor_format=) + torch against augment_batch(tensor_format=, view=).
The chain's result equals the view's bit for bit (checked once per shape before timing)."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/view_time.txt")
    ap.add_argument("--shapes", default="512x1024:896,4096x256:224")
    ap.add_argument("--collections", type=int, default=5)
    args = ap.parse_args()
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

    def row(label, t, bytes_moved=None):
        tail = "   %.2f TB/s" % (bytes_moved / (t[0] * 1e-3) / 1e12) if bytes_moved else ""
        return "  %-86s %8.3f ms  (min %.3f, max %.3f)%s" % (label, t[0], t[1], t[2], tail)

    nz = stainlib_amd.MacenkoNormalizer()
    nz.fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]])[0].cpu().numpy())
    f16 = stainlib_amd.TensorFormat(dtype=torch.float16, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    lines = ["device %s; ms per call: median of %d collections, each the median of 20 single launches by HIP events after a 0.25 s spin-up"
             % (torch.cuda.get_device_name(0), args.collections)]
    for shape in args.shapes.split(","):
        n, size, crop = (int(x) for x in shape.replace(":", "x").split("x"))
        wpx = n * crop * crop
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
        small = rgb[:, :crop, :crop].contiguous()                       # the yardstick's tiles: as many pixels as the view writes
        u8s = torch.empty_like(small)
        t16s = torch.empty((n, 3, crop, crop), dtype=torch.float16, device=dev)
        t16v = torch.empty_like(t16s)
        t16c = torch.empty_like(t16s)
        t16 = torch.empty((n, 3, size, size), dtype=torch.float16, device=dev)
        ws = engine.Workspace()
        # the torch half of the chain: per code the tiles that drew it, one gather of their windows, flip / rot90, into the batch
        groups = []
        for d in sorted(set(win[:, 2].tolist())):
            idx = np.nonzero(win[:, 2] == d)[0]
            ar = torch.arange(crop, device=dev)
            groups.append((d, torch.from_numpy(idx).to(dev), torch.from_numpy(idx).to(dev)[:, None, None, None],
                           torch.arange(3, device=dev)[None, :, None, None],
                           (torch.from_numpy(win[idx, 0]).to(dev).long()[:, None] + ar)[:, None, :, None],
                           (torch.from_numpy(win[idx, 1]).to(dev).long()[:, None] + ar)[:, None, None, :]))

        def torch_half(x, out):
            for d, idx, ti, ci, ys, xs in groups:
                v = x[ti, ci, ys, xs]
                if d & 4:
                    v = torch.flip(v, dims=(3,))
                out[idx] = torch.rot90(v, d & 3, dims=(2, 3))
            return out

        def chain_pass():
            return torch_half(engine.normalize_jitter(rgb, M, maxC, Mt, ct, ab, fmt=f16, out=t16), t16c)

        def chain_full():
            return torch_half(nz.augment_batch(rgb, ab, out=t16, ws=ws, tensor_format=f16)[0], t16c)

        def view_pass(fmt, out):
            return engine.normalize_view(rgb, dwin, crop, 7, M, maxC, Mt, ct, ab, fmt=fmt, out=out)

        assert torch.equal(chain_pass(), view_pass(f16, t16v)), "the chain and the view disagree"
        u8v = view_pass(None, None)
        lines += ["", "%d tiles of %d^2 -> %d^2 (%.1f Mpx written of %.1f), codes %s" % (n, size, crop, wpx / 1e6, n * size * size / 1e6, sorted(
            set(win[:, 2].tolist())))]
        rates = {}
        for name, bpp, fmt, ys_out, v_out in (("float16 NCHW", 9, f16, t16s, t16v), ("uint8", 6, None, u8s, u8v)):
            ta = timed(lambda: engine.normalize_jitter(small, M, maxC, Mt, ct, ab, fmt=fmt, out=ys_out))
            tb = timed(lambda: view_pass(fmt, v_out))
            lines.append(row("1. k_apply_jitter on %d tiles of %d^2 -> %s, %d B/px" % (n, crop, name, bpp), ta, bpp * wpx))
            lines.append(row("   sl_normalize_view %d^2 -> %d^2 -> %s, %d B per window px" % (size, crop, name, bpp), tb, bpp * wpx))
            rates[name] = ta[0] / tb[0]
            lines.append("   the view runs at %.2f of k_apply_jitter's bytes/s" % rates[name])
        tc, tv = timed(chain_pass), timed(lambda: view_pass(f16, t16v))
        lines.append(row("2. chain: sl_normalize_jitter on the full tiles -> float16 NCHW, then torch crop / flip / rot90", tc))
        lines.append(row("   sl_normalize_view -> the same tensor", tv))
        lines.append("   the view takes %.2f of the chain's time" % (tv[0] / tc[0]))
        tcf = timed(chain_full)
        tvf = timed(lambda: nz.augment_batch(rgb, ab, out=t16v, ws=ws, tensor_format=f16, view=view, windows=dwin))
        lines.append(row("   with the fit: augment_batch(tensor_format=) + torch", tcf))
        lines.append(row("   with the fit: augment_batch(tensor_format=, view=)", tvf))
        del rgb, small, u8s, t16s, t16v, t16c, t16, ws, groups, u8v
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
