"""Writes HEIF bytes from Annex-B streams (tests/streamgen.py): single `hvc1` items and `grid` items over tile items
that share one `hvcC`, with every box version p265_amd/heif.py reads (infe v2 / v3, iloc v0-2, pitm v0 / v1, iref v0 / v1,
ipma v0 / v1 with 7- and 15-bit indices), both grid field widths, `mdat` (32-bit, 64-bit and to-the-end sizes) and `idat`
construction, several extents per item and 1 / 2 / 4-byte NAL lengths.  Test infrastructure: a writer of exactly what the
tests need, not a general muxer."""
import struct

START = b"\x00\x00\x00\x01"


def split_nals(stream):
    """The NAL units (without start codes) of an Annex-B stream that uses 4-byte start codes only."""
    parts = stream.split(START)
    assert parts[0] == b""
    return parts[1:]


def access_units(stream):
    """-> (parameter-set NALs, [NALs of each picture]): a picture starts at a VCL NAL with first_slice_segment_in_pic."""
    ps, aus = [], []
    for n in split_nals(stream):
        t = (n[0] >> 1) & 63
        if t in (32, 33, 34):
            ps.append(n)
        elif t < 32 and n[2] & 0x80:
            aus.append([n])
        else:
            aus[-1].append(n)
    return ps, aus


def box(typ, payload, size64=False, to_end=False):
    if to_end:
        return struct.pack(">I4s", 0, typ) + payload
    if size64:
        return struct.pack(">I4sQ", 1, typ, 16 + len(payload)) + payload
    return struct.pack(">I4s", 8 + len(payload), typ) + payload


def full(typ, version, flags, payload):
    return box(typ, struct.pack(">I", version << 24 | flags) + payload)


def hvcc(ps, length_size=4, chroma_format=1, bit_depth=8):
    h = bytearray(22)
    h[0] = 1
    h[1] = 2 if bit_depth > 8 else 1
    h[12] = 120
    h[13], h[15] = 0xF0, 0xFC
    h[16] = 0xFC | chroma_format
    h[17] = h[18] = 0xF8 | (bit_depth - 8)
    h[21] = 0x0C | (length_size - 1)
    arrays = {}
    for n in ps:
        arrays.setdefault((n[0] >> 1) & 63, []).append(n)
    out = bytes(h) + bytes([len(arrays)])
    for t in sorted(arrays):
        out += bytes([0x80 | t]) + struct.pack(">H", len(arrays[t]))
        for n in arrays[t]:
            out += struct.pack(">H", len(n)) + n
    return box(b"hvcC", out)


def length_prefixed(nals, length_size=4):
    return b"".join(len(n).to_bytes(length_size, "big") + n for n in nals)


def ispe(w, h):
    return full(b"ispe", 0, 0, struct.pack(">II", w, h))


def pixi(bits):
    return full(b"pixi", 0, 0, bytes([len(bits)] + list(bits)))


def colr_nclx(primaries, transfer, matrix, full_range):
    return box(b"colr", b"nclx" + struct.pack(">HHHB", primaries, transfer, matrix, 0x80 if full_range else 0))


def colr_icc(data, kind=b"prof"):
    return box(b"colr", kind + data)


def irot(angle):
    return box(b"irot", bytes([angle & 3]))


def imir(axis):
    return box(b"imir", bytes([axis & 1]))


def auxc(urn):
    return full(b"auxC", 0, 0, urn.encode() + b"\0")


def clap(w, h, horiz=(0, 1), vert=(0, 1)):
    return box(b"clap", struct.pack(">IIIIiIiI", w, 1, h, 1, horiz[0], horiz[1], vert[0], vert[1]))


def clap_rect(x, y, w, h, iw, ih):
    """The clap box of the rectangle (x, y, w, h) of an iw x ih image."""
    return clap(w, h, (2 * x + w - iw, 2), (2 * y + h - ih, 2))


def grid_payload(rows, cols, w, h, big=False):
    return bytes([0, 1 if big else 0, rows - 1, cols - 1]) + struct.pack(">II" if big else ">HH", w, h)


class Item:
    def __init__(self, iid, typ, data=b"", props=(), refs=None, method=0, extents=1):
        self.id, self.type, self.data, self.props = iid, typ, data, list(props)      # props: (box bytes, essential)
        self.refs, self.method, self.extents = refs or {}, method, extents


def build(items, primary, brands=(b"heic", b"mif1"), infe_version=2, iloc_version=1, pitm_version=0, iref_version=0,
          ipma_version=0, ipma_wide=False, mdat="32", extra_top=b""):
    """The file.  mdat: "32" | "64" | "end" (box size forms)."""
    ftyp = box(b"ftyp", brands[0] + struct.pack(">I", 0) + b"".join(brands))
    # ipco: every distinct property once
    ipco, index = [], {}
    for it in items:
        for p, _ in it.props:
            if p not in index:
                index[p] = len(ipco) + 1
                ipco.append(p)
    ipma = struct.pack(">I", sum(1 for it in items if it.props))
    for it in items:
        if not it.props:
            continue
        ipma += struct.pack(">H" if ipma_version == 0 else ">I", it.id) + bytes([len(it.props)])
        for p, ess in it.props:
            ipma += struct.pack(">H", (0x8000 if ess else 0) | index[p]) if ipma_wide else bytes([(0x80 if ess else 0) | index[p]])
    iprp = box(b"iprp", box(b"ipco", b"".join(ipco)) + full(b"ipma", ipma_version, 1 if ipma_wide else 0, ipma))
    infe = b""
    for it in items:
        infe += full(b"infe", infe_version, 0, struct.pack(">H" if infe_version == 2 else ">I", it.id) + b"\0\0" +
                     it.type.encode() + b"\0")
    iinf = full(b"iinf", 0, 0, struct.pack(">H", len(items)) + infe)
    iref = b""
    for it in items:
        for typ, to in it.refs.items():
            w = ">H" if iref_version == 0 else ">I"
            iref += box(typ.encode(), struct.pack(w, it.id) + struct.pack(">H", len(to)) + b"".join(struct.pack(w, t) for t in to))
    iref = full(b"iref", iref_version, 0, iref) if iref else b""
    hdlr = full(b"hdlr", 0, 0, b"\0\0\0\0pict" + b"\0" * 12 + b"\0")
    pitm = full(b"pitm", pitm_version, 0, struct.pack(">H" if pitm_version == 0 else ">I", primary))
    idat_data = b"".join(it.data for it in items if it.method == 1)
    idat = box(b"idat", idat_data) if idat_data else b""

    def meta(mdat_at):
        loc = b""
        at = {0: mdat_at, 1: 0}
        for it in items:
            loc += struct.pack(">H" if iloc_version < 2 else ">I", it.id)
            if iloc_version > 0:
                loc += struct.pack(">H", it.method)
            loc += struct.pack(">H", 0)                                  # data_reference_index; base_offset_size 0
            n = max(1, min(it.extents, len(it.data))) if it.data else 1
            cuts = [len(it.data) * k // n for k in range(n + 1)]
            zeros = getattr(it, "zero_extents", 0)              # (malformed on purpose: extents of offset 0, length 0)
            loc += struct.pack(">H", zeros or n)
            for k in range(zeros):
                loc += struct.pack(">II", 0, 0)
            for k in range(0 if zeros else n):
                loc += struct.pack(">II", at[it.method] + cuts[k], cuts[k + 1] - cuts[k])
            at[it.method] += len(it.data)
        head = struct.pack(">H", 0x4400) + struct.pack(">H" if iloc_version < 2 else ">I", len(items))
        iloc = full(b"iloc", iloc_version, 0, head + loc)
        return full(b"meta", 0, 0, hdlr + pitm + iinf + iref + iprp + idat + iloc)

    if iloc_version == 0:
        assert all(it.method == 0 for it in items), "iloc v0 has no construction method"
    mhead = 16 if mdat == "64" else 8
    m = meta(0)
    m = meta(len(ftyp) + len(extra_top) + len(m) + mhead)
    payload = b"".join(it.data for it in items if it.method == 0)
    return ftyp + extra_top + m + box(b"mdat", payload, size64=mdat == "64", to_end=mdat == "end")


def single_file(stream, size, transforms=(), colr=None, length_size=4, bit_depth=8, chroma_format=1, **kw):
    """One hvc1 item holding the stream's first picture.  transforms: property boxes in order."""
    ps, aus = access_units(stream)
    props = [(hvcc(ps, length_size, chroma_format, bit_depth), True), (ispe(*size), False)]
    if colr is not None:
        props.append((colr, False))
    props += [(t, True) for t in transforms]
    item_kw = {k: kw.pop(k) for k in ("method", "extents") if k in kw}
    return build([Item(1, "hvc1", length_prefixed(aus[0], length_size), props, **item_kw)], 1, **kw)


def grid_items(stream, rows, cols, out_size, tile_size, first_id, transforms=(), colr=None, extra=(), length_size=4,
               bit_depth=8, chroma_format=1, grid_big=False, grid_method=0, tile_method=0, extents=1):
    """[grid item, tile items...] with ids first_id, first_id + 1 ...; the stream holds rows * cols pictures."""
    ps, aus = access_units(stream)
    assert len(aus) == rows * cols
    hv = hvcc(ps, length_size, chroma_format, bit_depth)
    tiles = [Item(first_id + 1 + k, "hvc1", length_prefixed(au, length_size), [(hv, True), (ispe(*tile_size), False)],
                  method=tile_method, extents=extents) for k, au in enumerate(aus)]
    props = [(ispe(*out_size), False)] + ([(colr, False)] if colr is not None else []) + [(p, False) for p in extra]
    props += [(t, True) for t in transforms]
    grid = Item(first_id, "grid", grid_payload(rows, cols, out_size[0], out_size[1], grid_big), props,
                refs={"dimg": [t.id for t in tiles]}, method=grid_method)
    return [grid] + tiles


def grid_file(stream, rows, cols, out_size, tile_size, alpha_stream=None, alpha_kw=None, build_kw=None, **kw):
    items = grid_items(stream, rows, cols, out_size, tile_size, 1, **kw)
    if alpha_stream is not None:
        akw = dict(kw, transforms=kw.get("transforms", ()), colr=None,
                   extra=[auxc("urn:mpeg:mpegB:cicp:systems:auxiliary:alpha")])
        akw.update(alpha_kw or {})
        a = grid_items(alpha_stream, rows, cols, out_size, tile_size, 100, **akw)
        a[0].refs["auxl"] = [1]
        items += a
    return build(items, 1, **(build_kw or {}))
