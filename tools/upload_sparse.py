"""Dense against sparse coefficient upload at the benchmark's picture mix, in one process on one GPU.

    python tools/upload_sparse.py [--pictures N] [--bit-depth B] [--repeats R] [--device D]

Builds the C3 synthetic mix bench.py uses (synth.make_picture(..., perf=True), 4 distinct 1080p pictures
replicated to N), uploads it dense (p265r_batch_upload) and sparse (p265r_batch_upload_sparse, pictures
sparsified beforehand) alternately -- one warm-up each, then R timed repeats -- and prints one JSON line:
upload_bytes, upload wall time (median, min, max), the expand kernels' time (HIP events), the host
sparsify time (p265r_sparsify, one thread, separately) and coef_nonzero_frac.  The sparse batch's device
digests (output and reconstruction) are checked against the dense batch's before anything is printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from p265_amd import recon, synth  # noqa: E402
from p265_amd import records as R  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=512)
    ap.add_argument("--bit-depth", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unique", type=int, default=4)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.repeats < 5:
        ap.error("--repeats: at least 5")
    params = R.make_params(pic_width=1920, pic_height=1080, bit_depth_luma=a.bit_depth, bit_depth_chroma=a.bit_depth)
    uniq = [synth.make_picture(params, 268 + i, perf=True) for i in range(a.unique)]
    t_sp = []
    usp = []
    for p in uniq:
        t0 = time.perf_counter()
        usp.append(recon.sparsify(p))
        t_sp.append(time.perf_counter() - t0)
    pics = [uniq[i % a.unique] for i in range(a.pictures)]
    sps = [usp[i % a.unique] for i in range(a.pictures)]
    coded = sum(p.n_coded_coef for p in uniq)
    nnz = sum(int(np.count_nonzero(p.coef)) for p in uniq)
    with recon.ReconContext(params, device=a.device) as ctx:
        ctx.set_timing(True)                            # (the sparse upload then times its expand kernels)
        digests, nbytes = {}, {}
        wall = {"dense": [], "sparse": []}
        expand = []
        for rep in range(a.repeats + 1):                # rep 0: warm-up (allocations, pinned staging, kernels)
            for kind, src in (("dense", pics), ("sparse", sps)):
                t0 = time.perf_counter()
                b = ctx.upload(src, sparse=kind == "sparse")
                dt = time.perf_counter() - t0
                if rep == 0:
                    nbytes[kind] = ctx.upload_bytes(b)
                    ctx.run(b)
                    digests[kind] = (ctx.digest(b), ctx.digest(b, recon=True))
                else:
                    wall[kind].append(dt * 1e3)
                    if kind == "sparse":
                        expand.append(float(ctx.describe()["last_sparse_expand_ms"]))
                b.free()
    for k in (0, 1):
        if not np.array_equal(digests["dense"][k], digests["sparse"][k]):
            raise SystemExit("sparse upload: device digests differ from the dense upload's")

    def stats(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    n_ctu = sum(len(p.ctus) for p in pics)
    out = {"tool": "upload_sparse", "pictures": a.pictures, "bit_depth": a.bit_depth, "repeats": a.repeats,
           "ctus": n_ctu, "coef_nonzero_frac": round(nnz / max(1, coded), 3),
           "upload_bytes": nbytes, "bytes_ratio": round(nbytes["sparse"] / nbytes["dense"], 4),
           "upload_ms": {k: stats(v) for k, v in wall.items()},
           "expand_kernels_ms": stats(expand),
           "sparsify_ms_per_picture": round(statistics.median(t_sp) * 1e3, 3),
           "sparsify_ms_batch_one_thread": round(statistics.median(t_sp) * 1e3 * a.pictures, 1),
           "digests_equal": True}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
