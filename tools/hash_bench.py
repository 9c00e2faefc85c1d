#!/usr/bin/env python3
"""Time of the device-side picture hash (p265r_batch_hash_async) on resident 1080p pictures, beside its yardsticks.

Per bit depth (8, 10) and batch size (8, 512) it uploads and runs the batch, then times ``--reps`` (20) hashes
per type between p265r_sync calls (host clock around work that ends in a device synchronise; one untimed call
first).  In the same process and on the same batches: p265r_batch_digest_async (the project's own digest, which
reads the same bytes in the same grid shape), libp265probe.so's read rate, and what the decoder does with
hash_on="host": download() plus bitstream.plane_hash of every plane on a 16-thread pool.  ``--e2e`` adds
decode_file of 128 x 1080p with export nv12, hash_on host against device, three interleaved repetitions.
Prints one JSON line per measurement.  A measurement tool: needs the GPU and fails without one.

    python tools/hash_bench.py [--frames 8,512] [--depths 8,10] [--reps 20] [--e2e] [--device 0]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = {0: "md5", 1: "crc", 2: "checksum"}


def probe_read_gbs(device, nbytes):
    lib = ctypes.CDLL(os.path.join(ROOT, "p265_amd", "libp265probe.so"))
    fn = lib.p265probe_stream
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.POINTER(ctypes.c_double)] * 3
    c, r, w = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    rc = fn(device, float(nbytes), ctypes.byref(c), ctypes.byref(r), ctypes.byref(w))
    if rc:
        raise RuntimeError("p265probe_stream = %d" % rc)
    return r.value


def timed(ctx, enqueue, reps):
    enqueue()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        enqueue()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def resident(a, out):
    from p265_amd import bitstream, recon, synth
    from p265_amd import records as R
    w, h = 1920, 1080
    pool = ThreadPoolExecutor(max_workers=16)
    for bd in a.depths:
        params = R.make_params(pic_width=w, pic_height=h, bit_depth_luma=bd, bit_depth_chroma=bd)
        uniq = [synth.make_picture(params, 268 + i, perf=True) for i in range(a.unique)]
        pic_bytes = w * h * 3 // 2 * (2 if bd > 8 else 1)
        for n in a.frames:
            pics = [uniq[i % a.unique] for i in range(n)]
            with recon.ReconContext(params, device=a.device) as ctx:
                batch = ctx.upload(pics)
                ctx.run(batch)
                ctx.status(batch)
                base = {"bit_depth": bd, "pictures": n, "plane_bytes": pic_bytes * n}
                ms = timed(ctx, lambda: ctx.digest_async(batch, 0), a.reps)
                out(dict(base, what="digest_async", ms=round(ms, 4), gbs=round(pic_bytes * n / ms / 1e6, 1)))
                for t in (2, 1, 0):
                    ms = timed(ctx, lambda: ctx.hash_async(batch, t), a.reps)
                    out(dict(base, what="hash_async " + NAMES[t], ms=round(ms, 4), gbs=round(pic_bytes * n / ms / 1e6, 1)))
                # the host leg: download + the host hash of every plane on 16 threads
                planes = ctx.download(batch)
                for t in (0,) if n > 8 else (0, 1, 2):
                    best = None
                    for _ in range(a.host_reps):
                        t0 = time.perf_counter()
                        planes = ctx.download(batch, into=planes)
                        t1 = time.perf_counter()
                        got = list(pool.map(lambda p: bitstream.plane_hash(p, t), [p for pic in planes for p in pic]))
                        t2 = time.perf_counter()
                        if best is None or t2 - t0 < best[0]:
                            best = (t2 - t0, t1 - t0, t2 - t1)
                    dev = ctx.picture_hash(batch, t)
                    assert [x for pic in dev for x in pic] == got, "device hash differs from the host hash"
                    out(dict(base, what="host download + 16-thread " + NAMES[t], ms=round(best[0] * 1e3, 3),
                             download_ms=round(best[1] * 1e3, 3), hash_ms=round(best[2] * 1e3, 3), d2h_bytes=pic_bytes * n))
                del planes
                batch.free()
    pool.shutdown()


def end_to_end(a, out):
    import tempfile
    from p265_amd import bitstream, decoder, recon
    one = open(os.path.join(ROOT, "tests", "golden", "synth_1080p_4pic.bin"), "rb").read()
    reps = 32
    n_ctu = reps * sum(len(p.picture.ctus) for p in bitstream.decode_stream(one))
    spec = recon.ExportSpec.named("nv12")
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(one * reps)
        f.flush()
        for mode in ("host", "device"):
            decoder.decode_file(f.name, None, export=spec, hash_on=mode)            # warm: contexts, kernels
        for rep in range(3):
            for mode in ("host", "device"):
                t0 = time.perf_counter()
                st = decoder.decode_file(f.name, None, export=spec, hash_on=mode)
                dt = time.perf_counter() - t0
                assert st["pictures"] == 4 * reps and st["hash_checked"] == 4 * reps and st["hash_mismatch"] == 0
                d2h = st["pictures"] * (1920 * 1080 * 3 // 2 if mode == "host" else 48)
                out({"what": "decode_file 128 x 1080p export nv12", "hash_on": mode, "rep": rep, "s": round(dt, 4),
                     "ctu_per_s": round(n_ctu / dt), "d2h_bytes": d2h})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="8,512")
    ap.add_argument("--depths", default="8,10")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--unique", type=int, default=2, help="distinct synthetic pictures (repeated to the batch size)")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--probe-bytes", type=float, default=float(4 << 30))
    a = ap.parse_args(argv)
    a.frames = [int(v) for v in a.frames.split(",") if v]
    a.depths = [int(v) for v in a.depths.split(",") if v]
    from p265_amd import recon
    if recon.device_count() < 1:
        raise SystemExit("hash_bench: no HIP device")

    def out(row):
        print(json.dumps(row), flush=True)

    out({"what": "probe read rate", "gbs": round(probe_read_gbs(a.device, a.probe_bytes), 1), "how": "p265probe_stream"})
    resident(a, out)
    if a.e2e:
        end_to_end(a, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
