"""Command line decoder, mirroring the reference's ``p265`` script (p265:7-20):

    python -m p265_amd.dec -b sanity.bin -o out.yuv

``-b/--bitstream`` and ``-o/--output`` keep the reference's meaning (its ``-o`` is
declared but never written, p265:9); ``--skip-syntax-dump`` is accepted for command
line compatibility (this decoder writes no syntax logs).  Parsing runs on host threads
(libp265fe.so), reconstruction on the MI355X (libp265r.so); the file is streamed
(bounded memory) and the YUV written in output order as pictures complete.  ``--format nv12|p010|rgb24|
rgb-planar-f16`` (with ``--matrix``, ``--full-range``, ``--upsample`` for RGB) converts on the GPU and writes the
exported frames; the default ``i420`` is the host path.  ``--hash-on device`` checks the decoded picture hash SEI
on the GPU instead of on downloaded planes.  A monochrome (4:0:0) stream writes luma-only frames by default;
``--mono-output i420`` appends chroma planes of 1 << (BitDepth - 1), and the GPU formats take their one-plane
forms (nv12 / p010: a grey CbCr plane; RGB: R = G = B).  ``--resize WxH`` (with ``--resize-filter nearest|bilinear|
area``) scales every frame of a GPU format to that size on the GPU (the scaled device-side output); the default
``i420`` host path does not scale and refuses both.  A stream whose luma and chroma bit depths differ takes the
``i420`` host path with ``--hash-on host`` only (the GPU formats and the GPU hash refuse it by name); when either
depth exceeds 8 its file holds every plane as 16-bit little-endian samples, values unscaled.
``--heif in.heic`` (instead of ``-b``) decodes a HEIF / HEIC still image: the grid is assembled, cut and oriented on the
GPU (``--no-orientation`` ignores irot / imir), every ``--format`` is a GPU format there, ``--probe`` prints the
container's description only.  ``--resize WxH --resize-filter ...`` scales it on the GPU too (the scaled grid export) and
then takes several files, of any grid shape, window and orientation over one set of sequence parameters: their
frames, all W x H, are written one after another.
"""
import argparse
import sys
import time

from . import decoder
from . import recon

FORMATS = ("i420", "nv12", "p010", "rgb24", "rgb-planar-f16")


def parse_cmd(argv=None):
    ap = argparse.ArgumentParser(prog="p265_amd.dec")
    ap.add_argument("-b", "--bitstream", help="The h.265 bitstream to be decoded.")
    ap.add_argument("--heif", metavar="FILE", nargs="+",
                    help="A HEIF / HEIC still image to be decoded instead (p265_amd.heif): its primary item, grid assembled "
                    "and orientation applied on the GPU; --format i420 is the GPU's planar form.  With --resize several "
                    "files (one set of sequence parameters and tile size) are decoded into frames of that one size, "
                    "written one after another")
    ap.add_argument("--no-orientation", action="store_true", help="--heif: ignore irot / imir")
    ap.add_argument("--probe", action="store_true", help="--heif: print the container's description and decode nothing")
    ap.add_argument("-o", "--output", help="The reconstructed output (--format, default I420; cropped, output order).")
    ap.add_argument("--skip-syntax-dump", type=int, default=0, help="Accepted for compatibility; no effect.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0, help="front-end parsing threads (0 = this process's CPU share, <= 16)")
    ap.add_argument("--batch", type=int, default=decoder.DEFAULT_BATCH, help="pictures per GPU batch")
    ap.add_argument("--depth", type=int, default=decoder.DEFAULT_DEPTH, help="GPU batches in flight (one warm context each)")
    ap.add_argument("--sparse-upload", action="store_true",
                    help="upload the coefficients as their non-zero levels, expanded on the GPU (same output)")
    ap.add_argument("--no-verify", action="store_true", help="do not fail on a decoded picture hash mismatch")
    ap.add_argument("--hash-on", choices=("host", "device"), default="host",
                    help="where the decoded picture hash SEI is checked: on downloaded planes (host) or on the GPU "
                         "(device: 48 bytes per picture come back; with a GPU --format no plane does)")
    ap.add_argument("--format", choices=FORMATS, default="i420",
                    help="output format; anything but i420 is converted on the GPU (cropped, device-side output) and "
                         "copied back once per batch")
    ap.add_argument("--matrix", choices=("bt601", "bt709", "bt2020"), default=None,
                    help="RGB formats: the YCbCr matrix (default bt709; --heif: the file's colour description unless "
                         "--matrix or --full-range is given)")
    ap.add_argument("--full-range", action="store_true", help="RGB formats: full-range YCbCr (default limited)")
    ap.add_argument("--upsample", choices=("nearest", "bilinear"), default="nearest", help="RGB formats: chroma upsampling")
    ap.add_argument("--mono-output", choices=("y", "i420"), default="y",
                    help="a monochrome (4:0:0) stream with the default --format: luma-only frames (y), or I420 frames "
                         "whose chroma planes are 1 << (BitDepth - 1) (i420)")
    ap.add_argument("--resize", metavar="WxH", default=None,
                    help="GPU formats: scale every (cropped) frame to W x H on the GPU")
    ap.add_argument("--resize-filter", choices=("nearest", "bilinear", "area"), default=None,
                    help="the filter of --resize (default bilinear; area: exact box average, downscale only)")
    a = ap.parse_args(argv)
    a.colour_given = a.matrix is not None or a.full_range      # (--heif: the command line's colour wins over the file's)
    if a.matrix is None:
        a.matrix = "bt709"
    if (a.bitstream is None) == (a.heif is None):
        ap.error("one of -b/--bitstream and --heif is required")
    if a.heif is not None and len(a.heif) > 1 and (a.resize is None or a.probe):
        ap.error("--heif: several files need --resize WxH (frames of one size)")
    if a.resize is not None or a.resize_filter is not None:
        if a.format == "i420" and a.heif is None:
            ap.error("--resize / --resize-filter scale on the GPU: choose a GPU --format (%s); the default i420 is the "
                     "host path and does not scale" % ", ".join(FORMATS[1:]))
        if a.resize is None:
            ap.error("--resize-filter needs --resize WxH")
        try:
            w, h = (int(v) for v in a.resize.lower().split("x"))
        except ValueError:
            ap.error("--resize: WxH, e.g. 224x224")
        a.resize = (w, h)
    return a


def export_spec(a):
    """The ExportSpec of the parsed command line; None for the default i420 (the host path, unchanged)."""
    if a.format == "i420":
        return None
    kw = {}
    if a.resize is not None:
        kw = dict(size=a.resize, resize=a.resize_filter or "bilinear")
    return recon.ExportSpec.named(a.format, matrix=a.matrix, full_range=a.full_range, upsample=a.upsample, **kw)


def heif_main(a):
    """--heif: probe, or decode the primary item(s) and write the oriented (--resize: scaled) frames' planes, rows tight."""
    from . import heif
    if a.probe:
        print(heif.probe(a.heif[0]))
        return 0
    kw = dict(size=a.resize, resize=a.resize_filter or "bilinear") if a.resize is not None else {}
    named = recon.ExportSpec.named(a.format, matrix=a.matrix, full_range=a.full_range, upsample=a.upsample, **kw)
    imgs = heif.decode_many(a.heif, export=named, device=a.device, apply_orientation=not a.no_orientation, aux=(),
                            verify_hash=not a.no_verify, hash_on=a.hash_on, colour="spec" if a.colour_given else "file")
    if a.output:
        with open(a.output, "wb") as f:
            for img in imgs:
                f.write(img.frames.slot(img.index).tobytes())
    for img in imgs:
        print({"width": img.width, "height": img.height, "bit_depth": img.bit_depth, "orientation": img.orientation,
               "colour": img.colour, "format": a.format, "icc": img.icc is not None})
    imgs[0].frames.free()
    return 0


def main(argv=None):
    a = parse_cmd(argv)
    if a.heif is not None:
        return heif_main(a)
    t0 = time.time()
    st = decoder.decode_file(a.bitstream, a.output, device=a.device, batch=a.batch, threads=a.threads,
                             depth=a.depth, verify_hash=not a.no_verify, sparse_upload=a.sparse_upload,
                             export=export_spec(a), hash_on=a.hash_on, mono_output=a.mono_output)
    dt = time.time() - t0
    print("decoded %d pictures in %.3f s; picture hash SEI checked %d, mismatched %d"
          % (st["pictures"], dt, st["hash_checked"], st["hash_mismatch"]))
    return 1 if st["hash_mismatch"] else 0


if __name__ == "__main__":
    sys.exit(main())
