#!/usr/bin/env python3
"""Rate of the scaled device-side output (p265r_batch_export_resized) on resident 1080p pictures, beside the plain
full-size export of the same format and the HBM copy rate.

As tools/export_bench.py: uploads and runs ``--frames`` (512) 8-bit 1080p pictures, then times ``--reps`` (20) exports
per case between p265r_sync calls (host clock around work that ends in a device synchronise; one untimed export
first), and measures libp265probe.so's p265probe_stream copy rate in the same process.  Per case one JSON line: ms
per scaled export, ms of the PLAIN export of the same format on the same batch (the yardstick: that kernel reads the
same source bytes), their ratio, the source bytes the filter must touch (area: the whole window; nearest / bilinear:
1 / 4 taps per output sample and plane, counted without reuse) plus the bytes written, and the time as a fraction
of the probe's copy rate over those bytes.  A measurement tool: needs the GPU and fails without one.

    python tools/resize_bench.py [--frames 512] [--reps 20] [--unique 2] [--device 0]
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

# (name, ExportSpec fields of the format, output size, filter)
CASES = [("rgb-planar-f16 224x224 nearest", dict(format="rgb_planar", sample="f16"), (224, 224), "nearest"),
         ("rgb-planar-f16 224x224 bilinear", dict(format="rgb_planar", sample="f16"), (224, 224), "bilinear"),
         ("rgb-planar-f16 224x224 area", dict(format="rgb_planar", sample="f16"), (224, 224), "area"),
         ("rgb24 960x540 area", dict(format="rgb_packed", sample="u8"), (960, 540), "area"),
         ("nv12 960x540 bilinear", dict(format="semiplanar", sample="native"), (960, 540), "bilinear"),
         ("nv12 960x540 area", dict(format="semiplanar", sample="native"), (960, 540), "area")]


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


def timed(ctx, batch, spec, nbytes, reps):
    from p265_amd import hip
    buf = hip.DeviceBuffer(nbytes)
    try:
        ctx.export(batch, spec, dst=buf.ptr.value, dst_bytes=buf.nbytes)      # warm-up
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.export(batch, spec, dst=buf.ptr.value, dst_bytes=buf.nbytes)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        ctx.status(batch)
    finally:
        buf.free()
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unique", type=int, default=2, help="distinct synthetic pictures (repeated to --frames)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--probe-bytes", type=float, default=float(4 << 30))
    a = ap.parse_args(argv)
    from p265_amd import recon, synth
    from p265_amd import records as R
    if recon.device_count() < 1:
        raise SystemExit("resize_bench: no HIP device")
    copy_gbs = probe_copy_gbs(a.device, a.probe_bytes)
    print(json.dumps({"probe_copy_gbs": round(copy_gbs, 1), "how": "p265probe_stream, read + write bytes"}), flush=True)
    w, h = 1920, 1080
    params = R.make_params(pic_width=w, pic_height=h)
    uniq = [synth.make_picture(params, 268 + i, perf=True) for i in range(a.unique)]
    pics = [uniq[i % a.unique] for i in range(a.frames)]
    src_bytes = w * h * 3 // 2
    with recon.ReconContext(params, device=a.device) as ctx:
        batch = ctx.upload(pics)
        ctx.run(batch)
        ctx.status(batch)
        plain_ms = {}
        for name, kw, size, filt in CASES:
            key = tuple(sorted(kw.items()))
            if key not in plain_ms:
                plain = recon.ExportSpec(**kw)
                plain_ms[key] = timed(ctx, batch, plain, ctx.export_layout(plain).frame_bytes * a.frames, a.reps)
            spec = recon.ExportSpec(size=size, resize=filt, **kw)
            lay = ctx.export_layout(spec)
            ms = timed(ctx, batch, spec, lay.frame_bytes * a.frames, a.reps)
            rgb = kw["format"].startswith("rgb")
            outs = size[0] * size[1] * (3 if rgb else 1) + (0 if rgb else 2 * (size[0] // 2) * (size[1] // 2))
            taps = {"nearest": 1, "bilinear": 4}.get(filt)
            touched = src_bytes if taps is None else min(src_bytes, outs * taps)
            moved = (touched + lay.frame_bytes) * a.frames
            gbs = moved / (ms * 1e-3) / 1e9
            print(json.dumps({"case": name, "pictures": a.frames, "ms_per_export": round(ms, 4),
                              "plain_export_ms": round(plain_ms[key], 4), "fraction_of_plain_export": round(ms / plain_ms[key], 3),
                              "source_bytes_touched": touched * a.frames, "bytes_written": lay.frame_bytes * a.frames,
                              "gbs": round(gbs, 1), "fraction_of_copy_rate": round(gbs / copy_gbs, 3)}), flush=True)
        batch.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
