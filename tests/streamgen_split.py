"""Streams whose luma and chroma bit depths differ (BitDepthY != BitDepthC, Main 10 / format range extensions):
tests/streamgen.py's generator with an SPS that states the two depths.

The generator itself keeps one depth and runs at ``min(Y, C)``: every depth-dependent range it draws from (slice and
CU QP deltas, PCM sample depths, SAO offsets) is then legal for both components.  What it cannot know is how a
decoder with the real depths reads its syntax where the SEMANTICS depend on the depth (QpBdOffset in the QP wrap,
the PCM shift, the SAO offset scale), so its own records are not the stream's: the expected records are the ones
libp265fe.so parses, the expected planes the C oracle's on those records, and the decoded picture hash SEI is
computed from them (``stream()`` generates twice: once with placeholder hashes to parse, once with the real ones).

One element's BINARIZATION depends on the depth: sao_offset_abs is TR with cMax = (1 << (Min(bitDepth, 10) - 5)) - 1
of its component (7.3.8.3, 9.3.3.2).  The generator has one cMax, so SAO is coded only where Min(Y, 10) ==
Min(C, 10); elsewhere the stream has SAO off.
"""
import numpy as np

import streamgen
from streamgen import BitWriter, nal
from oracle import c_oracle
from p265_amd import bitstream


class StreamGenSplit(streamgen.StreamGen):
    def __init__(self, seed=0, depths=(8, 10), **cfg):
        self.depths = (int(depths[0]), int(depths[1]))
        cfg = dict(cfg)
        cfg["bit_depth"] = min(self.depths)
        if min(self.depths[0], 10) != min(self.depths[1], 10):
            cfg["sao"] = False
        self._seed, self._cfg = seed, dict(cfg)
        super().__init__(seed, **cfg)

    def _ptl(self, bw):
        # format range extensions profile (4), Main 12 constraint flags
        bw.u(0, 2); bw.u(0, 1); bw.u(4, 5)
        bw.u(0x08000000, 32)
        bw.u(0b1001, 4)
        for b in (1, 0, 0, 1, 1, 0, 0, 0, 1):            # max_12bit .. lower_bit_rate
            bw.u(b, 1)
        bw.u(0, 34); bw.u(0, 1)
        bw.u(120, 8)

    def sps(self):
        c = self.cfg
        bw = BitWriter()
        bw.u(0, 4); bw.u(0, 3); bw.u(1, 1)
        self._ptl(bw)
        bw.ue(0); bw.ue(1)
        bw.ue(self.W); bw.ue(self.H)
        if c["conf_window"]:
            bw.u(1, 1)
            for v in c["conf_window"]:
                bw.ue(v)
        else:
            bw.u(0, 1)
        bw.ue(self.depths[0] - 8); bw.ue(self.depths[1] - 8)      # bit_depth_luma / chroma_minus8: the two depths
        bw.ue(c["log2_max_poc_lsb"] - 4)
        bw.u(1, 1); bw.ue(1 + c["max_reorder"]); bw.ue(c["max_reorder"]); bw.ue(0)
        bw.ue(c["min_cb_log2"] - 3); bw.ue(c["ctb_log2"] - c["min_cb_log2"])
        bw.ue(c["min_tb_log2"] - 2); bw.ue(c["max_tb_log2"] - c["min_tb_log2"])
        bw.ue(c["max_th_depth"]); bw.ue(c["max_th_depth"])
        assert c["scaling_lists"] is None
        bw.u(0, 1)
        bw.u(1, 1); bw.u(int(c["sao"]), 1)
        if c["pcm"]:
            lo, hi, lfd = c["pcm"]
            bw.u(1, 1); bw.u(self.pcm_bd[0] - 1, 4); bw.u(self.pcm_bd[1] - 1, 4)    # (<= min(Y, C): legal for both)
            bw.ue(lo - 3); bw.ue(hi - lo); bw.u(int(lfd), 1)
        else:
            bw.u(0, 1)
        bw.ue(1)
        bw.ue(1); bw.ue(0); bw.ue(0); bw.u(1, 1)
        bw.u(0, 1); bw.u(0, 1); bw.u(int(c["strong"]), 1)
        bw.u(0, 1)                                       # vui_parameters_present_flag
        bw.u(0, 1)                                       # sps_extension_present_flag
        bw.trailing()
        return nal(33, bw.bytes())

    def hash_sei_placeholder(self):
        """As the base class, with fixed bytes: the placeholder must not draw from the picture syntax's generator
        (the second pass of stream() has to produce the same pictures)."""
        kind = {"md5": 0, "crc": 1, "checksum": 2}[self.cfg["hash_sei"]]
        ln = {0: 16, 1: 2, 2: 4}[kind]
        payload = bytes([kind]) + bytes([0x5a] * (3 * ln))
        self.last_hash = (kind, [payload[1 + i * ln: 1 + (i + 1) * ln] for i in range(3)])
        return streamgen.sei_nal(payload)

    def stream(self, planes_fn=None):
        """-> (bytes, [(params, records.Picture, poc)], [(recon planes, out planes)]): the params and records as
        libp265fe.so parses them from the stream, the planes as the C oracle decodes those records; a hash SEI
        (``hash_sei``) is of those output planes, each in its own sample width (D.3.19)."""
        assert planes_fn is None
        data, gen = super().stream()
        dec = bitstream.decode_stream(data, threads=2, validate=True)
        assert len(dec) == len(gen)
        refs = [c_oracle.decode(d.params, [d.picture], threads=2)[0] for d in dec]
        if self.cfg["hash_sei"]:
            again = StreamGenSplit(self._seed, depths=self.depths, **self._cfg)
            it = iter(refs)
            data2, _ = streamgen.StreamGen.stream(again, lambda params, pic: next(it)[1])
            dec2 = bitstream.decode_stream(data2, threads=2, validate=True)
            for a, b in zip(dec, dec2):                  # the same pictures, now with their real hashes
                assert a.params.tobytes() == b.params.tobytes() and np.array_equal(a.picture.tbs, b.picture.tbs)
                assert np.array_equal(a.picture.coef, b.picture.coef) and np.array_equal(a.picture.ctus, b.picture.ctus)
            data, dec = data2, dec2
        return data, [(d.params, d.picture, d.poc) for d in dec], refs
