#!/usr/bin/env python3
"""Rate of the device-side output (p265r_batch_export) on resident 1080p pictures, beside the HBM copy rate.

Uploads and runs ``--frames`` (512) 1080p pictures as the headline configuration of bench.py does, then times
``--reps`` (20) exports per format between p265r_sync calls (host clock around work that ends in a device
synchronise; one untimed export first), and measures libp265probe.so's p265probe_stream copy rate in the same
process.  Prints one JSON line per format: ms per export, bytes read + written (computed from the shapes) and
the fraction of the probe's copy rate.  A measurement tool: needs the GPU and fails without one.

    python tools/export_bench.py [--frames 512] [--reps 20] [--unique 2] [--device 0]
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

# (name, bit depth, ExportSpec fields)
FORMATS = [("nv12", 8, dict(format="semiplanar", sample="native")),
           ("p010", 10, dict(format="semiplanar", sample="msb16")),
           ("rgb-planar-f16-bilinear", 8, dict(format="rgb_planar", sample="f16", upsample="bilinear")),
           ("rgb24-nearest", 8, dict(format="rgb_packed", sample="u8", upsample="nearest"))]


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unique", type=int, default=2, help="distinct synthetic pictures (repeated to --frames)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--probe-bytes", type=float, default=float(4 << 30))
    a = ap.parse_args(argv)
    from p265_amd import hip, recon, synth
    from p265_amd import records as R
    if recon.device_count() < 1:
        raise SystemExit("export_bench: no HIP device")
    copy_gbs = probe_copy_gbs(a.device, a.probe_bytes)
    print(json.dumps({"probe_copy_gbs": round(copy_gbs, 1), "how": "p265probe_stream, read + write bytes"}), flush=True)
    w, h = 1920, 1080
    for bd in sorted({f[1] for f in FORMATS}):
        params = R.make_params(pic_width=w, pic_height=h, bit_depth_luma=bd, bit_depth_chroma=bd)
        uniq = [synth.make_picture(params, 268 + i, perf=True) for i in range(a.unique)]
        pics = [uniq[i % a.unique] for i in range(a.frames)]
        with recon.ReconContext(params, device=a.device) as ctx:
            batch = ctx.upload(pics)
            ctx.run(batch)
            ctx.status(batch)
            src_bytes = w * h * 3 // 2 * (2 if bd > 8 else 1)
            for name, fbd, kw in FORMATS:
                if fbd != bd:
                    continue
                spec = recon.ExportSpec(**kw)
                lay = ctx.export_layout(spec)
                buf = hip.DeviceBuffer(lay.frame_bytes * a.frames)
                try:
                    ctx.export(batch, spec, dst=buf.ptr.value, dst_bytes=buf.nbytes)      # warm-up
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        ctx.export(batch, spec, dst=buf.ptr.value, dst_bytes=buf.nbytes)
                    ctx.sync()
                    ms = (time.perf_counter() - t0) * 1e3 / a.reps
                    ctx.status(batch)
                finally:
                    buf.free()
                moved = (src_bytes + lay.frame_bytes) * a.frames
                gbs = moved / (ms * 1e-3) / 1e9
                print(json.dumps({"format": name, "bit_depth": bd, "pictures": a.frames, "ms_per_export": round(ms, 4),
                                  "bytes_read_plus_written": moved, "gbs": round(gbs, 1),
                                  "fraction_of_copy_rate": round(gbs / copy_gbs, 3)}), flush=True)
            batch.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
