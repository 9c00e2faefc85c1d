#!/usr/bin/env python3
"""Rate of the grid export (p265r_batch_export_grid) beside the plain export of the same pictures and the HBM copy
rate, and the wall-time split of heif.decode on a phone-sized file.

As tools/resize_bench.py: uploads and runs ``--frames`` x 48 8-bit pictures of 512 x 512 (synthetic, ``--unique``
distinct ones repeated), then times ``--reps`` exports per case between p265r_sync calls (host clock around work that
ends in a device synchronise; one untimed export first), and measures libp265probe.so's p265probe_stream copy rate in
the same process.  The grid is 6 rows x 8 columns with a 4032 x 3024 output.  Per format (packed uint8 RGB with bilinear
chroma, NV12, planar fp16 RGB) one JSON line for orientation 0 with the ms of p265r_batch_export of the same pictures
(the yardstick: the same source bytes, slots of 512 x 512 instead of one frame), and one line each for orientations 1
and 5 with their ratio to orientation 0; every line has the bytes read and written (a quarter turn: the staging pass
counted too) and the time as a fraction of the probe's copy rate over them.

``--heif`` (off by default: the tiles are written by tests/streamgen.py in Python, about 1.5 s each) writes a 48-tile
HEIF file with tests/heifgen.py and prints the mean of ``--heif-reps`` heif.decode calls split into container parse /
front-end / upload + run / export (HeifImage.timing), without picture-hash SEI.  A measurement tool: needs the GPU and
fails without one.

    python tools/grid_bench.py [--frames 8] [--reps 20] [--unique 4] [--device 0] [--heif]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS, COLS, TILE, OUT = 6, 8, 512, (4032, 3024)
CASES = [("rgb24 bilinear", dict(format="rgb_packed", sample="u8", upsample="bilinear")),
         ("nv12", dict(format="semiplanar", sample="native")),
         ("rgb-planar-f16", dict(format="rgb_planar", sample="f16"))]


def probe_copy_gbs(device, nbytes):
    lib = ctypes.CDLL(os.path.join(ROOT, "p265_amd", "libp265probe.so"))
    fn = lib.p265probe_stream
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.POINTER(ctypes.c_double)] * 3
    c, r, w = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    rc = fn(device, float(nbytes), ctypes.byref(c), ctypes.byref(r), ctypes.byref(w))
    if rc:
        raise RuntimeError("p265probe_stream = %d" % rc)
    return c.value


def timed(ctx, batch, call, nbytes, reps):
    from p265_amd import hip
    buf = hip.DeviceBuffer(nbytes)
    try:
        call(buf)                                                              # warm-up (and the staging allocation)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            call(buf)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        ctx.status(batch)
    finally:
        buf.free()
    return ms


def heif_split(device, reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import heifgen
    from streamgen import StreamGen
    from p265_amd import heif, recon
    t0 = time.perf_counter()
    g = StreamGen(4032, width=TILE, height=TILE, frames=ROWS * COLS, idr_period=1, ctb_log2=5, max_tb_log2=5)
    data = heifgen.grid_file(g.stream()[0], ROWS, COLS, OUT, (TILE, TILE))
    gen_s = time.perf_counter() - t0
    spec = recon.ExportSpec.named("rgb24", upsample="bilinear")
    heif.decode(data, export=spec, device=device).frames.free()                # warm-up
    tot, wall = {}, 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        img = heif.decode(data, export=spec, device=device)
        wall += time.perf_counter() - t0
        for k, v in img.timing.items():
            tot[k] = tot.get(k, 0.0) + v
        img.frames.free()
    line = {"case": "heif.decode 48 x 512 x 512 -> 4032 x 3024 rgb24", "file_bytes": len(data), "reps": reps,
            "wall_ms": round(wall / reps * 1e3, 2), "tile_generation_s": round(gen_s, 1)}
    line.update({k + "_ms": round(v / reps * 1e3, 2) for k, v in tot.items()})
    print(json.dumps(line), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8, help="4032 x 3024 frames per call (48 pictures each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic pictures (repeated to frames x 48)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--probe-bytes", type=float, default=float(4 << 30))
    ap.add_argument("--heif", action="store_true", help="also the heif.decode wall-time split (writes the tiles first)")
    ap.add_argument("--heif-reps", type=int, default=3)
    a = ap.parse_args(argv)
    from p265_amd import recon, synth
    from p265_amd import records as R
    if recon.device_count() < 1:
        raise SystemExit("grid_bench: no HIP device")
    copy_gbs = probe_copy_gbs(a.device, a.probe_bytes)
    print(json.dumps({"probe_copy_gbs": round(copy_gbs, 1), "how": "p265probe_stream, read + write bytes"}), flush=True)
    params = R.make_params(pic_width=TILE, pic_height=TILE)
    uniq = [synth.make_picture(params, 4032 + i, perf=True) for i in range(a.unique)]
    n = a.frames * ROWS * COLS
    pics = [uniq[i % a.unique] for i in range(n)]
    with recon.ReconContext(params, device=a.device) as ctx:
        batch = ctx.upload(pics)
        ctx.run(batch)
        ctx.status(batch)
        for name, kw in CASES:
            plain = recon.ExportSpec(**kw)
            play = ctx.export_layout(plain)
            plain_ms = timed(ctx, batch, lambda b: ctx.export(batch, plain, dst=b.ptr.value, dst_bytes=b.nbytes),
                             play.frame_bytes * n, a.reps)
            base = None
            for o in (0, 1, 5):
                grid = recon.GridSpec(ROWS, COLS, OUT[0], OUT[1], o)
                lay = ctx.grid_layout(plain, grid)
                ms = timed(ctx, batch, lambda b: ctx.export_grid(batch, plain, grid, dst=b.ptr.value, dst_bytes=b.nbytes),
                           lay.frame_bytes * a.frames, a.reps)
                base = ms if o == 0 else base
                src = OUT[0] * OUT[1] * 3 // 2
                out = lay.frame_bytes                                           # (tight: the bytes of one frame)
                moved = (src + out * (3 if o & 1 else 1)) * a.frames            # (a quarter turn: written, read, written)
                gbs = moved / (ms * 1e-3) / 1e9
                line = {"case": name, "orientation": o, "frames": a.frames, "ms_per_export": round(ms, 4),
                        "bytes_moved": moved, "gbs": round(gbs, 1), "fraction_of_copy_rate": round(gbs / copy_gbs, 3)}
                if o == 0:
                    line.update(plain_export_ms=round(plain_ms, 4), fraction_of_plain_export=round(ms / plain_ms, 3),
                                plain_export_bytes_written=play.frame_bytes * n, bytes_written=lay.frame_bytes * a.frames)
                else:
                    line["ratio_to_orientation_0"] = round(ms / base, 3)
                print(json.dumps(line), flush=True)
        batch.free()
    if a.heif:
        heif_split(a.device, a.heif_reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
