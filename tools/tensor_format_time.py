"""What the model-ready tensor output costs, beside the torch line it replaces.
    python tools/tensor_format_time.py [--out profiles/tensor_format_time.txt] [--shapes 512x1024,128x1024]
    python tools/tensor_format_time.py --u8-only --tree OTHER_CHECKOUT      (the uint8 transform_batch of another tree, appended to --out)
Device-resident synthetic tiles; float16 NCHW and float32 NCHW.  Every figure is the median of 20 launches timed one by one with HIP
events after a 0.25 s spin-up of the same call (min and max beside it).  Timed:
  1. the torch expression ((x.permute(0, 3, 1, 2).float() / 255) - mean) / std (then .to(dtype)) on an existing uint8 result
  2. sl_to_tensor alone; the fused sl_normalize_apply_tensor alone; k_apply (sl_normalize_apply) alone -- with their achieved TB/s at
     the bytes the algorithm moves (3 B/px read, 3 x element size written; k_apply 3 + 3)
  3. Macenko transform_batch (uint8) followed by sl_to_tensor          (route "convert")
  4. Macenko transform_batch(tensor_format=...) as fit + fused apply   (route "fused")
  5. pooled Macenko transform_shard: uint8 followed by sl_to_tensor, against tensor_format=
The default route of transform_batch(tensor_format=...) (normalizer.TENSOR_ROUTE) is the faster of 3 and 4 at 512 x 1024^2."""
import argparse
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/tensor_format_time.txt")
    ap.add_argument("--shapes", default="512x1024,128x1024")
    ap.add_argument("--tree", default=".")
    ap.add_argument("--u8-only", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import torch
    import stainlib_amd as sl
    from stainlib_amd import engine
    from tools.synth import synth_tiles

    def timed(fn, reps=20):
        """(median, min, max) ms of `reps` calls timed one by one, after a spin-up (the clocks ramp for ~25 ms)"""
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
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        return statistics.median(ms), min(ms), max(ms)

    def row(label, t, bytes_moved=None):
        s = "  %-58s %8.3f ms  (min %.3f, max %.3f)" % (label, t[0], t[1], t[2])
        if bytes_moved is not None:
            s += "   %.2f TB/s" % (bytes_moved / (t[0] * 1e-3) / 1e12)
        return s

    nrm = sl.MacenkoNormalizer()
    Mt, ct, st = engine.macenko_fit(synth_tiles(1, 512, 512, seed=1, M_true=[[0.55, 0.75, 0.35], [0.10, 0.95, 0.20]]))
    assert int(st[0]) == 0
    nrm.stain_matrix_target, nrm.maxC_target = Mt[0].cpu().numpy(), ct[0].cpu().numpy().reshape(1, 2)
    lines = ["%sdevice %s; ms per call, median of 20 single launches by HIP events after a 0.25 s spin-up"
             % (args.label + ": " if args.label else "", torch.cuda.get_device_name(0))]
    for shape in args.shapes.split(","):
        n, size = (int(x) for x in shape.split("x"))
        px = n * size * size
        rgb = synth_tiles(n, size, size, seed=9)
        u8 = torch.empty_like(rgb)
        ws = engine.Workspace()
        lines += ["", "%d tiles of %d^2 (%.1f Mpx)" % (n, size, px / 1e6)]
        t_u8 = timed(lambda: nrm.transform_batch(rgb, out=u8, ws=ws))
        lines.append(row("Macenko transform_batch, uint8", t_u8))
        if args.u8_only:
            continue
        from stainlib_amd.distributed import SlideNormalizer
        _, M, maxC, status = nrm.transform_batch(rgb, out=u8, ws=ws)
        assert int((status != 0).sum()) == 0
        Mt_d, ct_d = nrm._target_on(rgb.device)
        lines.append(row("k_apply alone (sl_normalize_apply), 6 B/px", timed(lambda: engine.normalize_apply(rgb, M, maxC, Mt_d, ct_d, out=u8)), 6 * px))
        pooled = SlideNormalizer(nrm, group=False, mode="pooled")
        t_pool_u8 = timed(lambda: pooled.transform_shard(rgb, out=u8))
        lines.append(row("pooled Macenko transform_shard, uint8", t_pool_u8))
        nrm.transform_batch(rgb, out=u8, ws=ws)
        for dtype in (torch.float16, torch.float32):
            fmt = sl.TensorFormat(dtype, False, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
            es = 2 if dtype == torch.float16 else 4
            x = torch.empty((n, 3, size, size), dtype=dtype, device=rgb.device)
            mean = torch.tensor(fmt.mean, dtype=torch.float32, device=rgb.device)
            std = torch.tensor(fmt.std, dtype=torch.float32, device=rgb.device)
            lines.append(" %s NCHW" % str(dtype).replace("torch.", ""))

            def torch_line():
                return (((u8.permute(0, 3, 1, 2).float() / 255) - mean[:, None, None]) / std[:, None, None]).to(dtype)
            lines.append(row("1. torch expression on a uint8 result", timed(torch_line)))
            t2 = timed(lambda: engine.to_tensor(u8, fmt, out=x))
            lines.append(row("2. sl_to_tensor alone, %d B/px" % (3 + 3 * es), t2, (3 + 3 * es) * px))
            lines.append(row("   sl_normalize_apply_tensor alone, %d B/px" % (3 + 3 * es),
                             timed(lambda: engine.normalize_apply_tensor(rgb, M, maxC, Mt_d, ct_d, fmt, out=x)), (3 + 3 * es) * px))
            t3 = timed(lambda: nrm.transform_batch(rgb, out=x, ws=ws, tensor_format=fmt, _tensor_route="convert"))
            lines.append(row("3. transform_batch (uint8) + sl_to_tensor   [route convert]", t3))
            t4 = timed(lambda: nrm.transform_batch(rgb, out=x, ws=ws, tensor_format=fmt, _tensor_route="fused"))
            lines.append(row("4. fit + fused apply                        [route fused]", t4))
            lines.append("     -> %s is faster (%.3f of the other)" % (("fused", t4[0] / t3[0]) if t4[0] <= t3[0] else ("convert", t3[0] / t4[0])))
            t5a = timed(lambda: engine.to_tensor(pooled.transform_shard(rgb, out=u8)[0], fmt, out=x))
            lines.append(row("5. pooled transform_shard (uint8) + sl_to_tensor", t5a))
            lines.append(row("   pooled transform_shard(tensor_format=)", timed(lambda: pooled.transform_shard(rgb, out=x, tensor_format=fmt))))
            del x
        del rgb, u8
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(args.out, "a" if args.u8_only else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
