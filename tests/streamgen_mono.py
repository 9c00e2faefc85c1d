"""Monochrome (chroma_format_idc 0, ChromaArrayType 0) streams: tests/streamgen.py's generator with the
ChromaArrayType = 0 branches of the syntax (7.3, 10/2014 and later):

  SPS           chroma_format_idc 0; bit_depth_chroma_minus8 and pcm_sample_bit_depth_chroma_minus1 are still coded
                (``sps_bit_depth_chroma``: any value -- it means nothing); conformance window in luma samples
  slice header  no slice_sao_chroma_flag; slice_cb / cr_qp_offset still coded when the PPS says so
  sao()         one component
  coding_unit   no intra_chroma_pred_mode; pcm_sample(): luma samples alone
  transform_tree / transform_unit
                no cbf_cb / cbf_cr; cbfChroma = 0 in the cu_qp_delta_abs condition; no chroma residual_coding(),
                no deferred 4x4 chroma pair at blkIdx 3
  SEI           decoded picture hash of one component

The records come from frontend.PictureBuilder with monochrome params (no chroma TB, no chroma SAO).  The entropy
coder, the residual syntax and everything else are the base class's.  ``chroma_format_idc`` 2 / 3 and
``separate_colour_plane`` write the SPS fields and the slice-header fields that follow from them (colour_plane_id,
slice_sao_chroma_flag) for the refusal tests: the slice data stays ChromaArrayType-0 syntax, which no parser gets to.
"""
import numpy as np

import streamgen
from streamgen import BitWriter, ceil_log2, nal, picture_hash, sei_nal
from p265_amd import frontend
from p265_amd import records as R


class StreamGenMono(streamgen.StreamGen):
    def __init__(self, seed=0, chroma_format_idc=0, separate_colour_plane=0, sps_bit_depth_chroma=None, **cfg):
        super().__init__(seed, **cfg)
        self.chroma_format_idc, self.separate_colour_plane = chroma_format_idc, separate_colour_plane
        self.sps_bd_c = self.bd if sps_bit_depth_chroma is None else sps_bit_depth_chroma
        kw = R.params_dict(self.params)
        kw.update(chroma_format_idc=0, bit_depth_chroma=self.bd, pps_cb_qp_offset=0, pps_cr_qp_offset=0)
        self.params = R.make_params(**kw)

    def _ptl(self, bw):
        # format range extensions profile (4), Monochrome 12 constraint flags
        bw.u(0, 2); bw.u(0, 1); bw.u(4, 5)
        bw.u(0x08000000, 32)
        bw.u(0b1001, 4)
        for b in (1, 0, 0, 1, 1, 1, 1, 0, 1):            # max_12bit .. lower_bit_rate
            bw.u(b, 1)
        bw.u(0, 34); bw.u(0, 1)
        bw.u(120, 8)

    def sps(self):
        c = self.cfg
        bw = BitWriter()
        bw.u(0, 4); bw.u(0, 3); bw.u(1, 1)
        self._ptl(bw)
        bw.ue(0); bw.ue(self.chroma_format_idc)
        if self.chroma_format_idc == 3:
            bw.u(self.separate_colour_plane, 1)
        bw.ue(self.W); bw.ue(self.H)
        if c["conf_window"]:
            bw.u(1, 1)
            for v in c["conf_window"]:                   # units of SubWidthC = SubHeightC = 1 luma sample
                bw.ue(v)
        else:
            bw.u(0, 1)
        bw.ue(self.bd - 8); bw.ue(self.sps_bd_c - 8)
        bw.ue(c["log2_max_poc_lsb"] - 4)
        bw.u(1, 1); bw.ue(1 + c["max_reorder"]); bw.ue(c["max_reorder"]); bw.ue(0)
        bw.ue(c["min_cb_log2"] - 3); bw.ue(c["ctb_log2"] - c["min_cb_log2"])
        bw.ue(c["min_tb_log2"] - 2); bw.ue(c["max_tb_log2"] - c["min_tb_log2"])
        bw.ue(c["max_th_depth"]); bw.ue(c["max_th_depth"])
        if c["scaling_lists"] is None:
            bw.u(0, 1)
        else:
            bw.u(1, 1)
            bw.u(int(self.sps_sld is not None), 1)
            if self.sps_sld is not None:
                self._write_sld(bw, self.sps_sld)        # (all six matrices of a size are coded at any chroma format)
        bw.u(1, 1); bw.u(int(c["sao"]), 1)
        if c["pcm"]:
            lo, hi, lfd = c["pcm"]
            bw.u(1, 1); bw.u(self.pcm_bd[0] - 1, 4); bw.u(min(self.pcm_bd[1], self.sps_bd_c) - 1, 4)
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

    # ----------------------------------------------------------------- stream, SEI
    def stream(self, planes_fn=None):
        """As the base class; ``planes_fn(params, picture)`` returns the decoded planes, of which the first (Y)
        is hashed."""
        one = None if planes_fn is None else (lambda *a, **k: list(planes_fn(*a, **k))[:1])
        return super().stream(one)

    def hash_sei_placeholder(self):
        kind = {"md5": 0, "crc": 1, "checksum": 2}[self.cfg["hash_sei"]]
        ln = {0: 16, 1: 2, 2: 4}[kind]
        payload = bytes([kind]) + bytes(self.rng.integers(0, 256, ln, dtype=np.uint8))
        self.last_hash = (kind, [payload[1:1 + ln]])
        return sei_nal(payload)

    # ----------------------------------------------------------------- slice header
    def _slice_params(self, start):
        h = super()._slice_params(start)
        h["sao_chroma"] = 0                              # not coded, inferred 0: sao() has one component
        return h

    def _header(self, bw, nal_type, poc_lsb, start, dep, h, entry_points):
        c = self.cfg
        n = self.wc * self.hc
        bw.u(int(start == 0), 1)
        if 16 <= nal_type <= 23:
            bw.u(0, 1)
        bw.ue(0)
        if start != 0:
            if any(d for _, d in (c["slices"] or [])):
                bw.u(int(dep), 1)
            bw.u(self.ts_to_rs[start], ceil_log2(n))
        if not dep:
            bw.ue(2)
            if self.separate_colour_plane:
                bw.u(0, 2)                               # colour_plane_id
            if nal_type not in (19, 20):
                bw.u(poc_lsb, c["log2_max_poc_lsb"])
                bw.u(1, 1)
            if c["sao"]:
                bw.u(h["sao_luma"], 1)                   # (ChromaArrayType 0: no slice_sao_chroma_flag)
                if self.chroma_format_idc and not self.separate_colour_plane:
                    bw.u(0, 1)                           # (the refusal streams: their ChromaArrayType is not 0)
            bw.se(h["qp"] - c["init_qp"])
            if c["slice_chroma_offsets"] is not None:
                bw.se(h["cb"]); bw.se(h["cr"])           # parsed and ignored
            if c["deblocking"] == "override":
                bw.u(h["override"], 1)
                if h["override"]:
                    bw.u(h["dbk_disabled"], 1)
                    if not h["dbk_disabled"]:
                        bw.se(h["beta"]); bw.se(h["tc"])
            if h.get("code_lf_across"):
                bw.u(h["lf_across"], 1)
        if c["tiles"] is not None or c["wpp"]:
            bw.ue(len(entry_points))
            if entry_points:
                ln = max(max(entry_points).bit_length(), 1)
                bw.ue(ln - 1)
                for e in entry_points:
                    bw.u(e - 1, ln)
        bw.trailing()

    # ----------------------------------------------------------------- coding unit / transform tree
    def _cu(self, x0, y0, log2, depth):
        c, r, enc = self.cfg, self.rng, self.enc
        size = 1 << log2
        mcb = c["min_cb_log2"]
        self.depth[y0 >> mcb:(y0 + size) >> mcb, x0 >> mcb:(x0 + size) >> mcb] = depth
        qg_log2 = c["ctb_log2"] - (c["qp_delta_depth"] or 0)
        qmask = (1 << qg_log2) - 1
        if (x0 & qmask) == 0 and (y0 & qmask) == 0:
            self.qp_delta_coded = False
            self.qp_delta = 0
            prev = self.h["qp"] if self.first_qg else self.last_qp
            self.first_qg = False
            cm = self.ctb - 1
            qa = self.qpmap[y0 >> mcb, (x0 - 1) >> mcb] if (x0 & cm) else prev
            qb = self.qpmap[(y0 - 1) >> mcb, x0 >> mcb] if (y0 & cm) else prev
            self.qg_pred = (qa + qb + 1) >> 1
        bypass = 0
        if c["bypass"]:
            bypass = int(r.random() < c["bypass_prob"])
            enc.decision(self._ctx("bypass"), bypass)
        nxn = 0
        if log2 == mcb:
            nxn = int(r.random() < c["nxn_prob"])
            enc.decision(self._ctx("part_mode"), 1 - nxn)
        pcm = 0
        if c["pcm"] and not nxn and c["pcm"][0] <= log2 <= c["pcm"][1]:
            pcm = int(r.random() < c["pcm_prob"])
            enc.terminate(pcm)
        modes = [1, 1, 1, 1]
        tus = []
        pcm_samples = None
        if pcm:
            self.ipm[y0 >> 2:(y0 + size) >> 2, x0 >> 2:(x0 + size) >> 2] = 1
            self.enc.bw.align_zero()
            pby = self.pcm_bd[0]
            v = r.integers(0, 1 << pby, (size, size))    # pcm_sample_luma alone
            for s in v.reshape(-1):
                self.enc.bw.u(int(s), pby)
            pcm_samples = [(v << (self.bd - pby)).astype(np.int16), None, None]
            self.enc.start()
        else:
            nparts = 4 if nxn else 1
            pb = size >> 1 if nxn else size
            flags, code = [], []
            for i in range(nparts):
                xp, yp = x0 + pb * (i & 1), y0 + pb * (i >> 1)
                cand = self._mpm(xp, yp)
                m = cand[int(r.integers(0, 3))] if r.random() < 0.5 else int(r.integers(0, 35))
                modes[i] = m
                self.ipm[yp >> 2:(yp + pb) >> 2, xp >> 2:(xp + pb) >> 2] = m
                if m in cand:
                    flags.append(1)
                    code.append(cand.index(m))
                else:
                    flags.append(0)
                    code.append(m - sum(1 for v in sorted(cand) if v < m))
            for f in flags:
                enc.decision(self._ctx("prev_intra"), f)
            for f, v in zip(flags, code):
                if f:
                    enc.bypass(int(v > 0))
                    if v > 0:
                        enc.bypass(int(v > 1))
                else:
                    enc.bypass_bits(v, 5)
            # (no intra_chroma_pred_mode)
            self.cu = dict(x=x0, y=y0, log2=log2, nxn=nxn, bypass=bypass, modes=modes, mode_c=0)
            self._tt(x0, y0, x0, y0, log2, 0, 0, 0, 0, tus)
        off = self.qp_off
        qpy = ((self.qg_pred + self.qp_delta + 52 + 2 * off) % (52 + off)) - off
        self.last_qp = qpy
        self.qpmap[y0 >> mcb:(y0 + size) >> mcb, x0 >> mcb:(x0 + size) >> mcb] = qpy
        self.builder.add_cu(x0, y0, log2, 1 if nxn else 0, modes, 0, qpy + off, 0, 0, tus,
                            bypass=bool(bypass), pcm=bool(pcm), pcm_samples=pcm_samples)

    def _tt(self, x0, y0, xb, yb, log2, depth, blk, pcb, pcr, tus):
        c, r, enc, cu = self.cfg, self.rng, self.enc, self.cu
        maxd = c["max_th_depth"] + cu["nxn"]
        if log2 <= c["max_tb_log2"] and log2 > c["min_tb_log2"] and depth < maxd and not (cu["nxn"] and depth == 0):
            sp = c["tf_split_prob"]
            split = int(r.random() < (sp[log2] if isinstance(sp, dict) else sp))
            enc.decision(self._ctx("split_tf", 5 - log2), split)
        else:
            split = int(log2 > c["max_tb_log2"] or (cu["nxn"] and depth == 0))
        # (no cbf_cb / cbf_cr: both inferred 0)
        if split:
            hs = 1 << (log2 - 1)
            for i, (dx, dy) in enumerate(((0, 0), (hs, 0), (0, hs), (hs, hs))):
                self._tt(x0 + dx, y0 + dy, x0, y0, log2 - 1, depth + 1, i, 0, 0, tus)
            return
        cbl = int(r.random() < c["cbf_prob"])
        enc.decision(self._ctx("cbf_luma", 1 if depth == 0 else 0), cbl)
        if cbl and c["qp_delta_depth"] is not None and not self.qp_delta_coded:      # cbfChroma = 0
            lim = 26 + self.qp_off // 2
            v = int(r.integers(-lim, lim)) if r.random() < 0.7 else 0
            if r.random() < 0.6:
                v = int(np.clip(v, -4, 4))
            a = abs(v)
            for i in range(min(a, 5)):
                enc.decision(self._ctx("qp_delta", 0 if i == 0 else 1), 1)
            if a < 5:
                enc.decision(self._ctx("qp_delta", 0 if a == 0 else 1), 0)
            else:
                s, k = a - 5, 0
                while s >= (1 << k):
                    enc.bypass(1)
                    s -= 1 << k
                    k += 1
                enc.bypass(0)
                enc.bypass_bits(s, k)
            if a:
                enc.bypass(int(v < 0))
            self.qp_delta_coded = True
            self.qp_delta = v
        half = 1 << (cu["log2"] - 1)
        mode_y = cu["modes"][((y0 - cu["y"]) >= half) * 2 + ((x0 - cu["x"]) >= half)] if cu["nxn"] else cu["modes"][0]
        t = dict(x=x0, y=y0, log2=log2, blk=blk, cbf=[cbl, 0, 0], tskip=[0, 0, 0], coef=[None, None, None])
        if cbl:
            t["coef"][0], t["tskip"][0] = self._residual(log2, 0, mode_y)
        tus.append(t)


def luma_hash(planes, kind):
    """[hash of Y]: the one-component decoded picture hash."""
    return picture_hash(list(planes)[:1], kind)
