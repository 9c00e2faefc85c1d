"""HEIF / HEIC still images (ISO/IEC 23008-12 over ISO/IEC 14496-12): the container, the `grid` derivation and the
orientation, decoded into device memory through ``ReconContext.export_grid``.  Pure Python, no dependency.

    info = heif.probe(data_or_path)
    img  = heif.decode(data_or_path, export=ExportSpec.named("rgb24"))
    imgs = heif.decode_many([...], export=...)

What is read: ``ftyp`` (brands heic, heix, mif1, heim, heis), ``meta`` with ``hdlr``, ``pitm``, ``iinf`` / ``infe`` (v2,
v3), ``iloc`` (v0-2, construction methods 0 = file and 1 = ``idat``, several extents), ``iref`` (``dimg``, ``auxl``;
others ignored), ``iprp`` / ``ipco`` / ``ipma``, ``idat``; the properties ``hvcC``, ``ispe``, ``pixi``, ``colr``
(``nclx``; ``prof`` / ``rICC`` kept as bytes, never applied), ``irot``, ``imir``, ``auxC``, ``clap``; the items ``hvc1``
and ``grid``.  Everything else is refused BY NAME with ``UnsupportedHeif``; every malformed or truncated input raises
``HeifError`` (a ValueError) and nothing else.

Orientation is the back-end's: o = k | m << 2, np.rot90(F, k) then [:, ::-1].  ``irot`` angle a is k = a (anticlockwise
quarter turns); ``imir`` axis 0 mirrors about the vertical axis (left-right, o = 4), axis 1 about the horizontal axis
(top-bottom, o = 6).  Transformative properties apply in ``ipma`` order; any sequence reduces to one (window, o) through
the D4 table ``COMPOSE``.  A ``clap`` is folded into the window when it is integral (and starts on an even sample of a
4:2:0 image); after a turn it is mapped back into canvas coordinates.

Colour: ``colr nclx`` if present, else the SPS VUI (bitstream.DecodedPicture.colour), else BT.601 FULL range (the JFIF
convention still-image writers assume when they say nothing).  matrix_coeffs 1 -> bt709, 5 / 6 -> bt601, 9 -> bt2020,
2 (unspecified) -> the default; anything else (0 = identity / GBR included) is refused by name.
"""
import dataclasses
from fractions import Fraction

BRANDS = (b"heic", b"heix", b"mif1", b"heim", b"heis")
MAX_DEPTH, MAX_BOXES, MAX_ITEMS = 8, 1 << 16, 1 << 17
ALPHA_URNS = ("urn:mpeg:mpegB:cicp:systems:auxiliary:alpha", "urn:mpeg:hevc:2015:auxid:1")
DEPTH_URNS = ("urn:mpeg:mpegB:cicp:systems:auxiliary:depth", "urn:mpeg:hevc:2015:auxid:2")
START = b"\x00\x00\x00\x01"


class HeifError(ValueError):
    """A malformed or truncated file."""


class UnsupportedHeif(HeifError):
    """A well-formed file that asks for something outside this reader's scope (named in the message)."""


# o2 after o1: COMPOSE[o1][o2].  With r = a quarter turn anticlockwise and s = the left-right mirror, o stands for
# s^m r^k and r s = s r^-1, so (k1, m1) then (k2, m2) is k = k1 + (-1)^m1 k2 (mod 4), m = m1 ^ m2.
COMPOSE = (
    (0, 1, 2, 3, 4, 5, 6, 7),
    (1, 2, 3, 0, 5, 6, 7, 4),
    (2, 3, 0, 1, 6, 7, 4, 5),
    (3, 0, 1, 2, 7, 4, 5, 6),
    (4, 7, 6, 5, 0, 3, 2, 1),
    (5, 4, 7, 6, 1, 0, 3, 2),
    (6, 5, 4, 7, 2, 1, 0, 3),
    (7, 6, 5, 4, 3, 2, 1, 0),
)


def oriented_size(w, h, o):
    return (h, w) if o & 1 else (w, h)


def source_of(i, j, w, h, o):
    """(y, x) in a w x h array A of element [i][j] of the array oriented by o."""
    k, m = o & 3, o >> 2
    if m:
        j = oriented_size(w, h, o)[0] - 1 - j
    if k == 0:
        return i, j
    if k == 1:
        return j, w - 1 - i
    if k == 2:
        return h - 1 - i, w - 1 - j
    return h - 1 - j, i


def map_rect_back(rect, w, h, o):
    """A rectangle (x, y, cw, ch) of the oriented w x h array, as a rectangle of the array itself."""
    x, y, cw, ch = rect
    y0, x0 = source_of(y, x, w, h, o)
    y1, x1 = source_of(y + ch - 1, x + cw - 1, w, h, o)
    return min(x0, x1), min(y0, y1), abs(x1 - x0) + 1, abs(y1 - y0) + 1


class _Buf:
    """Bounds-checked big-endian reads of data[pos:end]."""

    def __init__(self, data, pos, end, what):
        if not 0 <= pos <= end <= len(data):
            raise HeifError("%s: range outside the file" % what)
        self.d, self.p, self.e, self.what = data, pos, end, what

    def left(self):
        return self.e - self.p

    def take(self, n):
        if n < 0 or n > self.e - self.p:
            raise HeifError("%s: truncated" % self.what)
        b = self.d[self.p:self.p + n]
        self.p += n
        return b

    def u(self, nbytes):
        return int.from_bytes(self.take(nbytes), "big") if nbytes else 0

    def s32(self):
        v = self.u(4)
        return v - (1 << 32) if v & 0x80000000 else v

    def full(self):
        v = self.u(4)
        return v >> 24, v & 0xFFFFFF

    def cstr(self):
        raw = bytes(self.d[self.p:self.e])
        i = raw.find(b"\0")
        if i < 0:
            raise HeifError("%s: unterminated string" % self.what)
        self.p += i + 1
        return raw[:i].decode("utf-8", "replace")


class _Budget:
    def __init__(self):
        self.boxes = 0

    def spend(self):
        self.boxes += 1
        if self.boxes > MAX_BOXES:
            raise HeifError("more than %d boxes" % MAX_BOXES)


def _boxes(data, pos, end, budget, depth, what):
    """[(type, payload start, payload end)] of the boxes in data[pos:end]: 32- and 64-bit sizes, size 0 = to the end."""
    if depth > MAX_DEPTH:
        raise HeifError("boxes nested deeper than %d" % MAX_DEPTH)
    out = []
    while pos < end:
        budget.spend()
        if end - pos < 8:
            raise HeifError("%s: truncated box header" % what)
        size, typ = int.from_bytes(data[pos:pos + 4], "big"), bytes(data[pos + 4:pos + 8])
        head = 8
        if size == 1:
            if end - pos < 16:
                raise HeifError("%s: truncated 64-bit box size" % what)
            size, head = int.from_bytes(data[pos + 8:pos + 16], "big"), 16
        elif size == 0:
            size = end - pos
        if size < head or size > end - pos:
            raise HeifError("%s: box %r of size %d does not fit its parent" % (what, typ, size))
        out.append((typ, pos + head, pos + size))
        pos += size
    return out


@dataclasses.dataclass
class Item:
    id: int
    type: str
    extents: list = dataclasses.field(default_factory=list)      # (construction method, offset, length)
    props: list = dataclasses.field(default_factory=list)        # (property dict, essential) in ipma order
    refs: dict = dataclasses.field(default_factory=dict)         # reference type -> [to ids]


def _prop(typ, data, a, b):
    """One ipco entry as a dict; unknown types keep only their name."""
    r = _Buf(data, a, b, typ.decode("latin1"))
    name = typ.decode("latin1")
    p = {"type": name}
    if typ == b"hvcC":
        raw = bytes(data[a:b])
        h = r.take(22)
        if h[0] != 1:
            raise HeifError("hvcC: configurationVersion %d" % h[0])
        p.update(raw=raw, chroma_format=h[16] & 3, bit_depth_luma=(h[17] & 7) + 8, bit_depth_chroma=(h[18] & 7) + 8,
                 length_size=(h[21] & 3) + 1, nals=[])
        for _ in range(r.u(1)):
            r.u(1)
            for _ in range(r.u(2)):
                p["nals"].append(bytes(r.take(r.u(2))))
    elif typ == b"ispe":
        r.full()
        p.update(width=r.u(4), height=r.u(4))
    elif typ == b"pixi":
        r.full()
        p.update(bits=[r.u(1) for _ in range(r.u(1))])
    elif typ == b"colr":
        kind = bytes(r.take(4))
        p["kind"] = kind.decode("latin1")
        if kind == b"nclx":
            p.update(primaries=r.u(2), transfer=r.u(2), matrix=r.u(2), full_range=bool(r.u(1) & 0x80))
        else:
            p["icc"] = bytes(r.take(r.left()))
    elif typ == b"irot":
        p["angle"] = r.u(1) & 3
    elif typ == b"imir":
        p["axis"] = r.u(1) & 1
    elif typ == b"auxC":
        r.full()
        p["urn"] = r.cstr()
    elif typ == b"clap":
        v = [r.u(4), r.u(4), r.u(4), r.u(4), r.s32(), r.u(4), r.s32(), r.u(4)]
        if 0 in (v[1], v[3], v[5], v[7]):
            raise HeifError("clap: zero denominator")
        p.update(width=Fraction(v[0], v[1]), height=Fraction(v[2], v[3]), horiz=Fraction(v[4], v[5]),
                 vert=Fraction(v[6], v[7]))
    else:
        p["unknown"] = True
    return p


class Container:
    """The parsed file: ``items`` {id: Item}, ``primary``, ``brands``, and the bytes the extents point into."""

    def __init__(self, data):
        self.data = data = memoryview(bytes(data))
        self.items, self.primary, self.brands, self.idat = {}, None, [], (0, 0)
        budget = _Budget()
        top = _boxes(data, 0, len(data), budget, 0, "file")
        if not top or top[0][0] != b"ftyp":
            raise HeifError("no ftyp box at the start of the file")
        r = _Buf(data, top[0][1], top[0][2], "ftyp")
        major = bytes(r.take(4))
        r.take(4)
        self.brands = [major] + [bytes(r.take(4)) for _ in range(r.left() // 4)]
        if not any(b in BRANDS for b in self.brands):
            if b"msf1" in self.brands or b"hevc" in self.brands:
                raise UnsupportedHeif("image sequence (brand msf1 / hevc): only still images are decoded")
            raise UnsupportedHeif("no HEIF still-image brand in ftyp (%s)" % b", ".join(self.brands).decode("latin1"))
        metas = [b for b in top if b[0] == b"meta"]
        if len(metas) != 1:
            raise HeifError("%d meta boxes at file level" % len(metas))
        self._meta(metas[0][1], metas[0][2], budget)

    def _meta(self, a, b, budget):
        data = self.data
        _Buf(data, a, b, "meta").full()
        kids = {}
        for typ, s, e in _boxes(data, a + 4, b, budget, 1, "meta"):
            kids.setdefault(typ, (s, e))
        if b"hdlr" in kids:
            r = _Buf(data, *kids[b"hdlr"], "hdlr")
            r.full()
            r.take(4)
            if bytes(r.take(4)) != b"pict":
                raise UnsupportedHeif("meta handler is not 'pict'")
        if b"iinf" not in kids or b"iloc" not in kids:
            raise HeifError("meta without iinf / iloc")
        self._iinf(*kids[b"iinf"], budget)
        if b"pitm" in kids:
            r = _Buf(data, *kids[b"pitm"], "pitm")
            v, _ = r.full()
            self.primary = r.u(2 if v == 0 else 4)
        if b"idat" in kids:
            self.idat = kids[b"idat"]
        self._iloc(*kids[b"iloc"])
        if b"iref" in kids:
            self._iref(*kids[b"iref"], budget)
        if b"iprp" in kids:
            self._iprp(*kids[b"iprp"], budget)
        if self.primary is None or self.primary not in self.items:
            raise HeifError("no primary item (pitm)")

    def _iinf(self, a, b, budget):
        r = _Buf(self.data, a, b, "iinf")
        v, _ = r.full()
        n = r.u(2 if v == 0 else 4)
        if n > MAX_ITEMS:
            raise HeifError("more than %d items" % MAX_ITEMS)
        for typ, s, e in _boxes(self.data, r.p, b, budget, 2, "iinf"):
            if typ != b"infe":
                continue
            q = _Buf(self.data, s, e, "infe")
            v, _ = q.full()
            if v < 2:
                raise UnsupportedHeif("infe version %d (items without a type)" % v)
            if v > 3:
                raise UnsupportedHeif("infe version %d" % v)
            iid = q.u(2 if v == 2 else 4)
            q.u(2)
            self.items[iid] = Item(iid, bytes(q.take(4)).decode("latin1"))
            if len(self.items) > MAX_ITEMS:
                raise HeifError("more than %d items" % MAX_ITEMS)

    def _iloc(self, a, b):
        r = _Buf(self.data, a, b, "iloc")
        v, _ = r.full()
        if v > 2:
            raise UnsupportedHeif("iloc version %d" % v)
        x = r.u(2)
        osz, lsz, bsz, isz = x >> 12, (x >> 8) & 15, (x >> 4) & 15, x & 15
        if any(s not in (0, 4, 8) for s in (osz, lsz, bsz)) or (v > 0 and isz not in (0, 4, 8)):
            raise HeifError("iloc: field size not 0, 4 or 8")
        n = r.u(2 if v < 2 else 4)
        if n > MAX_ITEMS:
            raise HeifError("more than %d iloc entries" % MAX_ITEMS)
        for _ in range(n):
            iid = r.u(2 if v < 2 else 4)
            method = r.u(2) & 15 if v > 0 else 0
            if r.u(2) != 0:
                raise UnsupportedHeif("iloc: data in another file (data_reference_index)")
            base = r.u(bsz)
            ext = []
            for _ in range(r.u(2)):
                if v > 0 and isz:
                    r.u(isz)
                off = r.u(osz)
                ext.append((method, base + off, r.u(lsz)))
            if method > 1:
                raise UnsupportedHeif("iloc construction method %d (item offsets)" % method)
            if iid in self.items:
                self.items[iid].extents = ext

    def _iref(self, a, b, budget):
        r = _Buf(self.data, a, b, "iref")
        v, _ = r.full()
        if v > 1:
            raise UnsupportedHeif("iref version %d" % v)
        w = 2 if v == 0 else 4
        for typ, s, e in _boxes(self.data, r.p, b, budget, 2, "iref"):
            q = _Buf(self.data, s, e, "iref entry")
            frm = q.u(w)
            to = [q.u(w) for _ in range(q.u(2))]
            if frm in self.items:
                self.items[frm].refs.setdefault(typ.decode("latin1"), []).extend(to)

    def _iprp(self, a, b, budget):
        kids = {}
        for typ, s, e in _boxes(self.data, a, b, budget, 2, "iprp"):
            kids.setdefault(typ, (s, e))
        if b"ipco" not in kids or b"ipma" not in kids:
            raise HeifError("iprp without ipco / ipma")
        props = [_prop(typ, self.data, s, e) for typ, s, e in _boxes(self.data, *kids[b"ipco"], budget, 3, "ipco")]
        r = _Buf(self.data, *kids[b"ipma"], "ipma")
        v, flags = r.full()
        for _ in range(r.u(4)):
            iid = r.u(2 if v == 0 else 4)
            for _ in range(r.u(1)):
                x = r.u(2) if flags & 1 else r.u(1)
                ess, idx = (x >> 15, x & 0x7FFF) if flags & 1 else (x >> 7, x & 0x7F)
                if idx == 0:
                    continue
                if idx > len(props):
                    raise HeifError("ipma: property index %d of %d" % (idx, len(props)))
                if iid in self.items:
                    self.items[iid].props.append((props[idx - 1], bool(ess)))

    # ---- item data ---------------------------------------------------------------------------------
    def item_bytes(self, item):
        out, total = [], 0
        for method, off, ln in item.extents:
            lo, hi = (0, len(self.data)) if method == 0 else self.idat
            if ln == 0:                                  # (the whole source, 8.11.3)
                ln = hi - lo - off
            if off < 0 or ln < 0 or lo + off + ln > hi:
                raise HeifError("item %d: extent outside %s" % (item.id, "the file" if method == 0 else "idat"))
            total += ln
            if total > len(self.data):                   # (extents that overlap: no item is larger than its file)
                raise HeifError("item %d: its extents add up to more than the file" % item.id)
            out.append(bytes(self.data[lo + off:lo + off + ln]))
        return b"".join(out)

    def prop(self, item, name):
        for p, _ in item.props:
            if p["type"] == name:
                return p
        return None


def _load(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def annexb(hvcc, data, what="item"):
    """Annex-B bytes of an hvc1 item's payload: a start code in front of every length-prefixed NAL unit."""
    n, out, p = hvcc["length_size"], [], 0
    while p < len(data):
        if len(data) - p < n:
            raise HeifError("%s: truncated NAL length" % what)
        ln = int.from_bytes(data[p:p + n], "big")
        p += n
        if ln > len(data) - p:
            raise HeifError("%s: NAL unit of %d bytes runs past the item" % (what, ln))
        out += [START, data[p:p + ln]]
        p += ln
    return b"".join(out)


def parameter_sets(hvcc):
    return b"".join(START + n for n in hvcc["nals"])


MATRICES = {1: "bt709", 5: "bt601", 6: "bt601", 9: "bt2020"}
DEFAULT_COLOUR = ("bt601", True)


def colour_of(matrix, full_range, what):
    """(matrix name, full_range) of a matrix_coeffs value; 2 = unspecified -> the default, with its range too."""
    if matrix == 2:
        return DEFAULT_COLOUR
    if matrix not in MATRICES:
        raise UnsupportedHeif("%s: matrix_coeffs %d (%s) is not supported" % (what, matrix, "identity / GBR" if matrix == 0 else "see H.273"))
    return (MATRICES[matrix], bool(full_range))


@dataclasses.dataclass
class ImageInfo:
    """One coded or derived image item, resolved: its tiles (hvc1 item ids, row-major), the canvas and the transforms."""
    id: int
    type: str
    width: int = 0              # the item's own (ispe / grid) size, before clap and orientation
    height: int = 0
    rows: int = 1
    cols: int = 1
    tiles: list = dataclasses.field(default_factory=list)
    tile_size: tuple = (0, 0)
    bit_depth: int = 8
    chroma_format: int = 1
    window: tuple = (0, 0, 0, 0)    # (x, y, w, h) on the canvas after every clap
    orientation: int = 0
    colour: object = None           # (matrix, full_range) from colr nclx, else None (the VUI / the default decide)
    icc: object = None
    aux_kind: object = None         # "alpha" | "depth" | the URN | None
    aux_of: object = None
    hvcc: object = None

    @property
    def size(self):
        return oriented_size(self.window[2], self.window[3], self.orientation)


def _resolve(c, item):
    """ImageInfo of an hvc1 or grid item.  Never recursive: the tiles of a grid must be hvc1 items themselves (a grid of
    derived images is refused), so a chain of dimg references is cut at its first link."""
    if item.type in ("iovl", "iden"):
        raise UnsupportedHeif("derived image item '%s' is not supported" % item.type)
    if item.type not in ("hvc1", "grid"):
        raise UnsupportedHeif("item type '%s' is not supported (HEVC 'hvc1' and 'grid' only)" % item.type)
    info = ImageInfo(item.id, item.type)
    ispe = c.prop(item, "ispe")
    if item.type == "hvc1":
        hv = c.prop(item, "hvcC")
        if hv is None or ispe is None:
            raise HeifError("item %d: hvc1 without hvcC / ispe" % item.id)
        info.width, info.height, info.tiles, info.tile_size = ispe["width"], ispe["height"], [item.id], (ispe["width"], ispe["height"])
        info.hvcc = hv
    else:
        d = c.item_bytes(item)
        r = _Buf(d, 0, len(d), "grid item %d" % item.id)
        if r.u(1) != 0:
            raise UnsupportedHeif("grid version other than 0")
        big = r.u(1) & 1
        info.rows, info.cols = r.u(1) + 1, r.u(1) + 1
        info.width, info.height = r.u(4 if big else 2), r.u(4 if big else 2)
        ids = item.refs.get("dimg", [])
        if len(ids) != info.rows * info.cols:
            raise HeifError("grid item %d: %d tiles for %d x %d" % (item.id, len(ids), info.rows, info.cols))
        first = None
        for t in ids:
            if t not in c.items:
                raise HeifError("grid item %d: tile %d does not exist" % (item.id, t))
            if t == item.id:
                raise HeifError("item %d refers to itself through dimg" % item.id)
            tile = c.items[t]
            if tile.type != "hvc1":
                raise UnsupportedHeif("grid of derived images (tile type '%s') is not supported" % tile.type)
            thv, tis = c.prop(tile, "hvcC"), c.prop(tile, "ispe")
            if thv is None or tis is None:
                raise HeifError("item %d: hvc1 without hvcC / ispe" % t)
            if first is None:
                first = (thv, (tis["width"], tis["height"]))
            elif thv["raw"] != first[0]["raw"]:
                raise UnsupportedHeif("grid tiles with differing hvcC configurations are not supported")
            elif (tis["width"], tis["height"]) != first[1]:
                raise UnsupportedHeif("grid tiles with differing ispe sizes are not supported")
        info.tiles, info.tile_size, info.hvcc = list(ids), first[1], first[0]
        tw, th = info.tile_size
        if not ((info.cols - 1) * tw < info.width <= info.cols * tw and (info.rows - 1) * th < info.height <= info.rows * th):
            raise HeifError("grid item %d: output %d x %d does not end in the last tile row / column" % (item.id, info.width, info.height))
    if info.width <= 0 or info.height <= 0:
        raise HeifError("item %d: empty image" % item.id)
    hv = info.hvcc
    info.bit_depth, info.chroma_format = hv["bit_depth_luma"], hv["chroma_format"]
    if hv["chroma_format"] > 1:
        raise UnsupportedHeif("chroma format 4:2:%s is not supported (4:2:0 and 4:0:0 only)" % ("2" if hv["chroma_format"] == 2 else "4 (4:4:4)"))
    if hv["chroma_format"] == 1 and hv["bit_depth_chroma"] != hv["bit_depth_luma"]:
        raise UnsupportedHeif("unequal luma / chroma bit depths are not supported")
    # properties in ipma order: descriptive ones are read, transformative ones composed
    x, y, w, h, o = 0, 0, info.width, info.height, 0
    for p, essential in item.props:
        t = p["type"]
        if t == "clap":
            ow, oh = oriented_size(w, h, o)
            cx, cy = Fraction(ow - 1, 2) + p["horiz"], Fraction(oh - 1, 2) + p["vert"]
            l, tp = cx - (p["width"] - 1) / 2, cy - (p["height"] - 1) / 2
            if any(v.denominator != 1 for v in (l, tp, p["width"], p["height"])):
                raise UnsupportedHeif("clap: a clean aperture that is not on whole samples is not supported")
            rect = (int(l), int(tp), int(p["width"]), int(p["height"]))
            if rect[0] < 0 or rect[1] < 0 or rect[2] <= 0 or rect[3] <= 0 or rect[0] + rect[2] > ow or rect[1] + rect[3] > oh:
                raise HeifError("clap: the clean aperture leaves the image")
            bx, by, bw, bh = map_rect_back(rect, w, h, o)
            x, y, w, h = x + bx, y + by, bw, bh
            if hv["chroma_format"] == 1 and ((x | y) & 1):
                raise UnsupportedHeif("clap: an odd left / top offset on a 4:2:0 image is not supported")
        elif t == "irot":
            o = COMPOSE[o][p["angle"]]
        elif t == "imir":
            o = COMPOSE[o][4 if p["axis"] == 0 else 6]
        elif t == "colr":
            if p["kind"] == "nclx":
                info.colour = colour_of(p["matrix"], p["full_range"], "colr nclx")
            else:
                info.icc = p["icc"]
        elif t == "auxC":
            info.aux_kind = "alpha" if p["urn"] in ALPHA_URNS else "depth" if p["urn"] in DEPTH_URNS else p["urn"]
        elif p.get("unknown") and essential:
            raise UnsupportedHeif("essential property '%s' is not supported" % t)
    info.window, info.orientation = (x, y, w, h), o
    return info


def probe(src):
    """-> {"primary": id, "brands": [...], "items": {id: dict}} for every image item that can be resolved (others:
    {"type": ..., "error": message})."""
    c = Container(_load(src))
    items = {}
    for iid, it in sorted(c.items.items()):
        if it.type not in ("hvc1", "grid", "iovl", "iden") and iid != c.primary:
            items[iid] = {"type": it.type}
            continue
        try:
            info = _resolve(c, it)
        except UnsupportedHeif as e:
            if iid == c.primary:
                raise
            items[iid] = {"type": it.type, "error": str(e)}
            continue
        items[iid] = {"type": info.type, "size": info.size, "coded_size": (info.width, info.height), "rows": info.rows,
                      "cols": info.cols, "tiles": info.tiles, "tile_size": info.tile_size, "bit_depth": info.bit_depth,
                      "chroma_format": info.chroma_format, "colour": info.colour, "orientation": info.orientation,
                      "window": info.window, "aux_kind": info.aux_kind,
                      "aux_of": (it.refs.get("auxl") or [None])[0],
                      "icc": info.icc is not None}
    return {"primary": c.primary, "brands": [b.decode("latin1") for b in c.brands], "items": items}


def item_stream(c, info):
    """The ONE Annex-B stream of an image item: the hvcC parameter sets once, then every tile's access unit."""
    out = [parameter_sets(info.hvcc)]
    for t in info.tiles:
        out.append(annexb(info.hvcc, c.item_bytes(c.items[t]), "item %d" % t))
    return b"".join(out)


@dataclasses.dataclass
class HeifImage:
    frames: object              # recon.DeviceFrames, one slot per image: the oriented image in device memory
    alpha: object
    width: int
    height: int
    bit_depth: int
    orientation: int
    colour: tuple
    icc: object
    timing: dict = dataclasses.field(default_factory=dict)
    index: int = 0              # decode_many: this image's slot in ``frames``
    source_size: object = None  # (width, height) of the oriented image before any resize; width / height are the slot's


def _parse(src, item, aux, apply_orientation):
    c = Container(_load(src))
    iid = c.primary if item is None else int(item)
    if iid not in c.items:
        raise HeifError("no item %d" % iid)
    info = _resolve(c, c.items[iid])
    if not apply_orientation:
        info.orientation = 0
    alpha = None
    if "alpha" in (aux or ()):
        for it in c.items.values():
            if iid in it.refs.get("auxl", []) and it.type in ("hvc1", "grid"):
                a = _resolve(c, it)
                if a.aux_kind == "alpha":
                    if a.chroma_format == 1 and ((a.window[2] | a.window[3]) & 1):
                        # (its Y plane comes out of a planar export, whose half-size planes need an even window)
                        raise UnsupportedHeif("an alpha auxiliary image coded 4:2:0 with an odd window is not supported "
                                              "(monochrome alpha images have no such limit)")
                    a.orientation = info.orientation
                    alpha = a
                    break
    return c, info, alpha


def _decode_items(jobs, export, device, verify_hash, hash_on, colour, timing):
    """jobs: [(container, ImageInfo)] of equally shaped images -- with ``export.size`` of any shape, over one set of
    sequence parameters -> (DeviceFrames of len(jobs) slots, colour)."""
    import time
    from . import bitstream, recon
    from . import records as R
    t0 = time.perf_counter()
    pics = []
    for c, info in jobs:
        dec = bitstream.decode_stream(item_stream(c, info))
        if len(dec) != len(info.tiles):
            raise HeifError("item %d: %d pictures in the stream of %d tiles" % (info.id, len(dec), len(info.tiles)))
        pics.append(dec)
    t1 = time.perf_counter()
    first, info0 = pics[0][0], jobs[0][1]
    for dec, (c, info) in zip(pics, jobs):
        for d in dec:
            if d.params.tobytes() != first.params.tobytes():
                raise UnsupportedHeif("images / tiles with differing sequence parameters cannot share a batch")
            if d.crop[0] or d.crop[2]:
                raise UnsupportedHeif("a conformance window with a left / top offset is not supported in a HEIF item")
        if export.size is None and (info.rows, info.cols, info.window, info.orientation, info.width, info.height) != \
                (info0.rows, info0.cols, info0.window, info0.orientation, info0.width, info0.height):
            raise UnsupportedHeif("decode_many: the images are not equally shaped")
    tw, th = int(first.params["pic_width"]), int(first.params["pic_height"])
    for _, info in (jobs if export.size is not None else jobs[:1]):
        if (tw - first.crop[1], th - first.crop[3]) != tuple(info.tile_size) and len(info.tiles) > 1:
            raise UnsupportedHeif("grid tiles whose conformance window differs from their coded size are not supported")
    if colour == "spec":
        col = (export.matrix, bool(export.full_range))
    elif info0.colour is not None:
        col = info0.colour
    elif first.colour is not None:
        col = colour_of(first.colour[0], first.colour[1], "SPS VUI")
    else:
        col = DEFAULT_COLOUR
    def crop_of(info):
        x, y, w, h = info.window
        return (x, info.width - x - w, y, info.height - y - h)
    if export.size is None:
        spec = dataclasses.replace(export, matrix=col[0], full_range=col[1], crop=crop_of(info0))
        grid = recon.GridSpec(info0.rows, info0.cols, info0.width, info0.height, info0.orientation)
    else:
        # one slot of export.size per image, whatever its grid, window or orientation (a single item: a 1 x 1 grid)
        spec = dataclasses.replace(export, matrix=col[0], full_range=col[1], crop=(0, 0, 0, 0))
        grid = [recon.GridFrame(info.rows, info.cols, info.width, info.height, crop_of(info), info.orientation)
                for _, info in jobs]
    flat = [d for dec in pics for d in dec]
    ctx = recon.ReconContext(first.params, device=device, scaling=first.scaling)
    try:
        batch = ctx.upload([d.picture for d in flat])
        ctx.run(batch)
        if verify_hash and any(d.hash for d in flat):
            _verify(ctx, batch, flat, hash_on, bitstream, R)
        ctx.status(batch)
        t2 = time.perf_counter()
        frames = ctx.export_grid(batch, spec, grid) if export.size is None else ctx.export_grid_resized(batch, spec, grid)
        ctx.status(batch)
        frames.detach()
        t3 = time.perf_counter()
        batch.free()
    finally:
        ctx.close()
    timing.update(frontend=timing.get("frontend", 0.0) + t1 - t0, upload_run=timing.get("upload_run", 0.0) + t2 - t1,
                  export=timing.get("export", 0.0) + t3 - t2)
    return frames, col


def _verify(ctx, batch, flat, hash_on, bitstream, R):
    if hash_on == "device":
        kinds = {d.hash_type for d in flat if d.hash}
        got = {k: ctx.picture_hash(batch, k) for k in kinds}
        for i, d in enumerate(flat):
            if d.hash and got[d.hash_type][i] != list(d.hash):
                raise HeifError("picture hash SEI mismatch (tile %d)" % i)
        return
    outs = ctx.download(batch)
    for i, d in enumerate(flat):
        if d.hash and [bitstream.plane_hash(p, d.hash_type) for p in outs[i][:len(d.hash)]] != list(d.hash):
            raise HeifError("picture hash SEI mismatch (tile %d)" % i)


def decode(src, export=None, device=0, item=None, aux=("alpha",), apply_orientation=True, verify_hash=True,
           hash_on="host", colour="file"):
    """Decode one image item (default: the primary) into device memory -> HeifImage.  ``colour`` "file": colr nclx, else
    the VUI, else BT.601 full range; "spec": ``export``'s own matrix / full_range.  ``aux`` ("alpha",): also decode the
    alpha auxiliary image (own context; planar, native samples, plane 0) with the same grid and orientation."""
    return decode_many([src], export=export, device=device, item=item, aux=aux, apply_orientation=apply_orientation,
                       verify_hash=verify_hash, hash_on=hash_on, colour=colour)[0]


def decode_many(srcs, export=None, device=0, item=None, aux=(), apply_orientation=True, verify_hash=True,
                hash_on="host", colour="file"):
    """Equally shaped images: one upload, one run, ONE grid-export call; -> [HeifImage] sharing one DeviceFrames of
    len(srcs) slots (``frames.batch_array()`` is the dense view), image i in slot ``index`` = i.  With ``export.size``
    (and ``resize``, ``scale``, ``bias``) the images may differ in grid shape, item size, clap window and orientation --
    grids and single items alike: every slot has that size (the scaled grid export); they must still share their
    sequence parameters and tile size, because they share one context."""
    import time
    from . import recon
    if export is None:
        export = recon.ExportSpec.named("rgb24")
    timing = {}
    t0 = time.perf_counter()
    parsed = [_parse(s, item, aux, apply_orientation) for s in srcs]
    if not parsed:
        return []
    timing["container"] = time.perf_counter() - t0
    with_alpha = all(a is not None for _, _, a in parsed)
    alpha_spec = recon.ExportSpec(format="planar")
    if export.size is not None and with_alpha:
        # the alpha image goes through the same call: planar, plane 0, the slot's size
        alpha_spec = recon.ExportSpec(format="planar", size=export.size, resize=export.resize)
        if any(a.chroma_format == 1 for _, _, a in parsed) and ((int(export.size[0]) | int(export.size[1])) & 1):
            raise UnsupportedHeif("an alpha auxiliary image coded 4:2:0 cannot be resized to an odd size %d x %d "
                                  "(monochrome alpha images have no such limit)" % (int(export.size[0]), int(export.size[1])))
    frames, col = _decode_items([(c, info) for c, info, _ in parsed], export, device, verify_hash, hash_on, colour, timing)
    alpha = None
    if with_alpha:
        alpha, _ = _decode_items([(c, a) for c, _, a in parsed], alpha_spec, device, verify_hash, hash_on, "file", timing)
    if export.size is not None:
        w, h = int(export.size[0]), int(export.size[1])
        return [HeifImage(frames, alpha, w, h, p[1].bit_depth, p[1].orientation, col, p[1].icc, timing, i, p[1].size)
                for i, p in enumerate(parsed)]
    info = parsed[0][1]
    w, h = info.size
    return [HeifImage(frames, alpha, w, h, info.bit_depth, info.orientation, col, p[1].icc, timing, i, (w, h))
            for i, p in enumerate(parsed)]
