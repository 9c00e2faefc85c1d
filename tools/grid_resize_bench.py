#!/usr/bin/env python3
"""Time of the scaled grid export (p265r_batch_export_grid_resized) beside its two yardsticks, both existing code:
p265r_batch_export_resized of an UNTILED 4032 x 3024 picture into the same output (the same arithmetic without the
tile table), and the full-size p265r_batch_export_grid (what a caller pays today before any resize).

As tools/grid_bench.py: uploads and runs ``--frames`` x 48 8-bit pictures of 512 x 512 (synthetic, ``--unique`` distinct
ones repeated) in one context and ``--frames`` pictures of 4032 x 3024 (one synthetic picture repeated) in another, then
times ``--reps`` exports per case between p265r_sync calls (host clock around work that ends in a device synchronise;
one untimed export first), and measures libp265probe.so's p265probe_stream copy rate in the same process.  The grid is
6 rows x 8 columns with a 4032 x 3024 item.  Outputs: planar fp16 RGB at 224 x 224 and packed uint8 RGB at 1008 x 756;
every filter at orientation 0 and orientation 1 (the twin has no orientation: its time is that of orientation 0's
arithmetic, with the turned size for orientation 1 so that it filters to the same pre-turn size).  One JSON line per
case.  A measurement tool: needs the GPU and fails without one.

    python tools/grid_resize_bench.py [--frames 4] [--reps 20] [--unique 4] [--device 0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grid_bench import COLS, OUT, ROWS, TILE, probe_copy_gbs, timed  # noqa: E402

CASES = [("rgb-planar-f16 224x224", dict(format="rgb_planar", sample="f16"), (224, 224)),
         ("rgb24 1008x756", dict(format="rgb_packed", sample="u8"), (1008, 756))]
FILTERS = ("nearest", "bilinear", "area")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4, help="4032 x 3024 frames per call (48 tiles each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic tiles (repeated to frames x 48)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--probe-bytes", type=float, default=float(4 << 30))
    a = ap.parse_args(argv)
    from p265_amd import recon, synth
    from p265_amd import records as R
    if recon.device_count() < 1:
        raise SystemExit("grid_resize_bench: no HIP device")
    copy_gbs = probe_copy_gbs(a.device, a.probe_bytes)
    print(json.dumps({"probe_copy_gbs": round(copy_gbs, 1), "how": "p265probe_stream, read + write bytes"}), flush=True)
    # ---- the untiled twin: the scaled export of whole 4032 x 3024 pictures
    twin = {}
    whole = R.make_params(pic_width=OUT[0], pic_height=OUT[1])
    pic = synth.make_picture(whole, 4033, perf=True)
    with recon.ReconContext(whole, device=a.device) as ctx:
        batch = ctx.upload([pic] * a.frames)
        ctx.run(batch)
        ctx.status(batch)
        for name, kw, size in CASES:
            for filt in FILTERS:
                for o in (0, 1):
                    spec = recon.ExportSpec(size=size[::-1] if o else size, resize=filt, **kw)
                    lay = ctx.export_layout(spec)
                    twin[name, filt, o] = timed(ctx, batch, lambda b: ctx.export(batch, spec, dst=b.ptr.value, dst_bytes=b.nbytes),
                                                lay.frame_bytes * a.frames, a.reps)
        batch.free()
    # ---- the grids
    params = R.make_params(pic_width=TILE, pic_height=TILE)
    uniq = [synth.make_picture(params, 4032 + i, perf=True) for i in range(a.unique)]
    pics = [uniq[i % a.unique] for i in range(a.frames * ROWS * COLS)]
    with recon.ReconContext(params, device=a.device) as ctx:
        batch = ctx.upload(pics)
        ctx.run(batch)
        ctx.status(batch)
        for name, kw, size in CASES:
            full = {}
            for o in (0, 1):
                plain, grid = recon.ExportSpec(**kw), recon.GridSpec(ROWS, COLS, OUT[0], OUT[1], o)
                lay = ctx.grid_layout(plain, grid)
                full[o] = timed(ctx, batch, lambda b: ctx.export_grid(batch, plain, grid, dst=b.ptr.value, dst_bytes=b.nbytes),
                                lay.frame_bytes * a.frames, a.reps)
            for filt in FILTERS:
                for o in (0, 1):
                    spec = recon.ExportSpec(size=size, resize=filt, **kw)
                    frames = [recon.GridFrame(ROWS, COLS, OUT[0], OUT[1], (0, 0, 0, 0), o)] * a.frames
                    lay = ctx.export_layout(spec)
                    ms = timed(ctx, batch, lambda b: ctx.export_grid_resized(batch, spec, frames, dst=b.ptr.value,
                                                                              dst_bytes=b.nbytes),
                               lay.frame_bytes * a.frames, a.reps)
                    t = twin[name, filt, o]
                    print(json.dumps({"case": name, "filter": filt, "orientation": o, "frames": a.frames,
                                      "ms_per_call": round(ms, 4), "untiled_resized_ms": round(t, 4),
                                      "ratio_to_untiled": round(ms / t, 3), "full_size_grid_ms": round(full[o], 4),
                                      "ratio_to_full_size_grid": round(ms / full[o], 3)}), flush=True)
        batch.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
