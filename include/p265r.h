/*
 * p265r.h -- C ABI of the MI355X (gfx950) HEVC intra reconstruction back-end.
 *
 * Drop-in boundary for the reconstruction hook of the p265 reference decoder.
 * The reference has no FFI: its boundary is the Python call
 *     Cu.parse -> Cu.decode_leaf()                 (decoder/cu.py:96-97, cu.py:483-494)
 * which (were it not dead, cu.py:487-488) would run, per leaf CU,
 *     Cu.decode_intra -> IntraPu.decode            (cu.py:595-615, intra.py:39-70)
 *       -> scaling.inverse_scaling                 (scaling.py:4-47)
 *       -> transform.inverse_transform             (transform.py:89-109)
 *       -> reconstruction.reconstruction           (reconstruction.py:4-27)
 * with the picture served back through Cu.get_reconstructed_sample (cu.py:617-632),
 * and the per-CTU SAO syntax of Sao.parse (sao.py:15-136) that nothing consumes.
 *
 * Here decode_leaf() only APPENDS records (one p265r_tb per transform block, one
 * p265r_ctu per CTU); at end of picture (slice.py:284-286) the host submits a batch
 * of pictures; the device runs dequant + inverse DCT/DST + intra prediction +
 * reconstruction + SAO and writes the decoded planes.  See INTEGRATION.md for the
 * ctypes binding the reference would add.
 *
 * Chroma formats: 4:2:0 (chroma_format_idc 1) and monochrome 4:0:0 (chroma_format_idc 0), BitDepth 8..12.
 * A monochrome context has no chroma anywhere -- every array keeps its shape, the chroma entries are not used:
 *   p265r_params    bit_depth_chroma, pps_cb / cr_qp_offset and the chroma entries of a scaling table are ignored
 *   records         a TB with c_idx != 0 or a non-zero sao_type[1..2] is P265R_EINVAL at upload, before any launch
 *   p265r_picture   out[1..2] and recon[1..2] are never read or written (P265R_PIC_RECON_INPUT takes recon[0] alone)
 *   p265r_batch_digest*     out[3 i + 1] = out[3 i + 2] = 0;  p265r_batch_hash_read: bytes 16..47 of a picture are 0
 *   p265r_batch_job_count   chroma = 0
 *   p265r_batch_export      P265R_FMT_PLANAR is the Y plane alone (the layout sets plane_off[1..2] = pitch[1..2] = 0);
 *                           P265R_FMT_SEMIPLANAR is Y plus a CbCr plane whose every element is 1 << (B - 1) (shifted
 *                           for MSB16): grey NV12 / P010; the RGB formats give R = G = B = clip((cy (Y - yoff) + 8192)
 *                           >> 14), the formula below at cb = cr = 0 (matrix and upsample are validated, otherwise
 *                           unused).  Crops may be odd for planar and RGB (SubWidthC = SubHeightC = 1); semi-planar
 *                           keeps the even rule of its 2 x 2-subsampled plane.
 *   p265r_describe  "chroma_format_idc", and "last_launch_layout" (the intra phase of the last run: "whole" |
 *                   "split" | "xg" | "luma" = the row kernel's luma-rows-only layout, which every monochrome
 *                   batch takes | "steps" | "none") with "last_launch_row_waves"
 * chroma_format_idc 2 and 3 are P265R_EINVAL from p265r_create.
 *
 * Unequal bit depths (BitDepthY != BitDepthC, Main 10 / RExt) are opt-in: p265r_params.split_bit_depth = 1.
 *   p265r_create    with the flag, bit_depth_luma and bit_depth_chroma are each 8..12 on their own; without it
 *                   unequal depths stay P265R_EUNSUPPORTED.  A value above 1 is P265R_EINVAL.  Monochrome ignores
 *                   the flag with the chroma depth; the flag with equal depths changes nothing.
 *   device planes   the context is WIDE when either depth exceeds 8: all three planes are then uint16_t in device
 *                   memory, whatever their own depth
 *   p265r_picture   out[c] / recon[c] (P265R_PIC_RECON_INPUT too) are typed per component: uint8_t for a component
 *                   of 8 bits, little-endian uint16_t above.  The 8-bit component of a wide context is narrowed on
 *                   the device before the download and widened on the host during the upload.
 *   p265r_batch_digest*     a wide context digests every plane in its 16-bit device form (an 8-bit component as
 *                           uint16_t samples: W/2 words of 2 samples per row)
 *   p265r_batch_export*     P265R_EINVAL (from the layout functions too);  p265r_batch_hash_async: P265R_EUNSUPPORTED
 *   p265r_describe  "bit_depth" (luma) and "bit_depth_chroma"
 *
 * Conventions: every function returns int (0 = P265R_OK, < 0 = error code, see
 * p265r_strerror); no exception or C++ type crosses this boundary.  All host
 * buffers are owned by the caller.  A context is bound to one device and is not
 * thread-safe: use one context per GPU per thread/process.
 */
#ifndef P265R_H
#define P265R_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P265R_ABI_VERSION 2u   /* 2: per-picture size in p265r_picture */

/* error codes */
#define P265R_OK            0
#define P265R_EINVAL       -1   /* bad argument / malformed record              */
#define P265R_ENOMEM       -2   /* host or device allocation failed             */
#define P265R_EHIP         -3   /* HIP runtime error (see p265r_last_hip_error) */
#define P265R_EUNSUPPORTED -4   /* stream feature outside this back-end's scope */
#define P265R_ERANGE       -5   /* record points outside picture / buffers      */
#define P265R_ESTATE       -6   /* call out of order (e.g. wait without submit) */
#define P265R_ENODEV       -7   /* no such HIP device                           */

/* p265r_tb.flags */
#define P265R_TB_CBF     0x01u  /* coefficients present at coef_off (N*N int16, raster)        */
#define P265R_TB_TSKIP   0x02u  /* transform_skip_flag (tu.py:142-143)                        */
#define P265R_TB_BYPASS  0x04u  /* cu_transquant_bypass_flag (cu.py:102-105)                 */
#define P265R_TB_PCM     0x08u  /* PCM block: coef holds samples at BitDepth; no prediction    */

/* p265r_picture.flags */
#define P265R_PIC_RECON_INPUT 0x01u /* recon[] holds the reconstruction (input): residual and intra
                                       phases are skipped, only the in-loop filters run (tile halo
                                       decoding, p265_amd/tiles.py).  All pictures of a batch must
                                       agree on this flag. */

/* p265r_ctu.flags */
#define P265R_CTU_LF_ACROSS_SLICES 0x01u  /* slice_loop_filter_across_slices_enabled_flag of its slice */
#define P265R_CTU_DEBLOCK          0x02u  /* deblocking on in its slice (!slice_deblocking_filter_disabled_flag,
                                             slice.py:170-175 / pps.py:122-131); 0 = the edges this CTU's
                                             coding blocks own (left/top/internal) are not filtered     */

/* p265r_ctu.deblock_offsets: slice_beta_offset_div2 in bits 0..3, slice_tc_offset_div2 in bits
 * 4..7, each a 4-bit two's-complement value in -6..6 (inherited from pps_*_offset_div2) */
#define P265R_DEBLOCK_OFFSETS(beta_div2, tc_div2) ((uint8_t)(((beta_div2) & 15) | (((tc_div2) & 15) << 4)))

/* Sequence-level parameters (SPS/PPS-derived fields the path reads; sps.py:59-62,
 * sps.py:142-171, sps.py:120, pps.py:38, pps.py:49-50).  POD, 32 bytes: RCCL-broadcastable. */
typedef struct p265r_params {
    uint32_t version;                 /* = P265R_ABI_VERSION                      */
    uint16_t pic_width;               /* pic_width_in_luma_samples                */
    uint16_t pic_height;              /* pic_height_in_luma_samples               */
    uint8_t  chroma_format_idc;       /* 1 (4:2:0) or 0 (4:0:0, monochrome)       */
    uint8_t  bit_depth_luma;          /* BitDepthY: 8, or 9..12 (uint16_t planes)   */
    uint8_t  bit_depth_chroma;        /* BitDepthC: equal to bit_depth_luma unless split_bit_depth
                                         (monochrome: ignored)                      */
    uint8_t  ctb_log2_size;           /* CtbLog2SizeY, 4..6                       */
    uint8_t  min_tb_log2_size;        /* MinTbLog2SizeY, 2..5                     */
    uint8_t  max_tb_log2_size;        /* MaxTbLog2SizeY, <= 5                     */
    uint8_t  strong_intra_smoothing;  /* strong_intra_smoothing_enabled_flag      */
    uint8_t  constrained_intra_pred;  /* constrained_intra_pred_flag (no effect: all-intra) */
    uint8_t  sample_adaptive_offset;  /* sample_adaptive_offset_enabled_flag      */
    uint8_t  loop_filter_across_tiles;/* loop_filter_across_tiles_enabled_flag    */
    uint8_t  scaling_list_enabled;    /* scaling_list_enabled_flag: 1 = dequantise with the ScalingFactor
                                         table given by p265r_set_scaling_factors (sps.py:86-90,
                                         scaling.py:32-44)                          */
    int8_t   pps_cb_qp_offset;        /* cQpPicOffset of Cb chroma deblocking (8.7.2.5.5) */
    int8_t   pps_cr_qp_offset;        /* cQpPicOffset of Cr chroma deblocking     */
    uint8_t  split_bit_depth;         /* 1: bit_depth_luma and bit_depth_chroma may differ, each 8..12;
                                         0: unequal depths are P265R_EUNSUPPORTED; > 1: P265R_EINVAL */
    uint8_t  reserved[10];
} p265r_params;

/* One CTU, raster order, PicSizeInCtbsY per picture.  32 bytes. */
typedef struct p265r_ctu {
    uint32_t tb_begin;        /* first p265r_tb of this CTU (its TBs are contiguous, decode order) */
    uint16_t tb_count;
    uint16_t tile_id;         /* TileId (tiles numbered in tile-scan order)                    */
    uint32_t slice_addr;      /* SliceAddrRs of the slice containing this CTU                  */
    uint8_t  flags;           /* P265R_CTU_*                                                   */
    uint8_t  sao_type[3];     /* SaoTypeIdx[cIdx]: 0 off, 1 band offset, 2 edge offset         */
    uint8_t  sao_class[3];    /* sao_band_position (type 1) or SaoEoClass (type 2)             */
    uint8_t  deblock_offsets; /* P265R_DEBLOCK_OFFSETS(slice_beta_offset_div2, slice_tc_offset_div2) */
    int8_t   sao_offset[3][4];/* SaoOffsetVal[cIdx][1..4]: signed, << log2OffsetScale          */
} p265r_ctu;

/* One transform block, in decode order within its CTU.  16 bytes.
 * Luma TBs of a TU precede its Cb and Cr TBs; for a luma 4x4 quad the single
 * 4x4 Cb/Cr pair follows blkIdx 3 (tu.py:127-135). */
typedef struct p265r_tb {
    uint16_t x, y;            /* top-left, in samples of component c_idx                       */
    uint8_t  log2_size;       /* 2..5                                                          */
    uint8_t  c_idx;           /* 0 Y, 1 Cb, 2 Cr                                               */
    uint8_t  pred_mode;       /* IntraPredModeY / IntraPredModeC, 0..34                        */
    uint8_t  flags;           /* P265R_TB_*                                                    */
    uint8_t  qp;              /* qP for scaling: Qp'Y or Qp'Cb / Qp'Cr (incl. QpBdOffset); luma
                                 TBs (PCM ones too) also give QpY + QpBdOffsetY to deblocking.
                                 0 .. 51 + 6 * (BitDepth of the component - 8), PCM TBs included:
                                 anything larger is P265R_EINVAL at upload                        */
    uint8_t  reserved[3];     /* 0; sparse upload: [0..1] = the TB's entry count, little-endian  */
    uint32_t coef_off;        /* int16 offset of the N*N TransCoeffLevel[y][x] (iff CBF|PCM);
                                 sparse upload, transformed TBs: index of the TB's first entry  */
} p265r_tb;

/* One picture of a batch (host memory, caller-owned). */
typedef struct p265r_picture {
    const p265r_ctu* ctus;    /* PicSizeInCtbsY entries, raster order                          */
    const p265r_tb*  tbs;
    uint32_t         n_tbs;
    uint32_t         flags;   /* P265R_PIC_*                                                   */
    const int16_t*   coef;
    uint64_t         n_coef;
    const uint8_t*   nofilter;/* optional (NULL): per 8x8 luma block, raster, ceil(W/8) wide;
                                 1 = deblocking and SAO leave the block's samples untouched
                                 (pcm_loop_filter_disabled && pcm, or cu_transquant_bypass)   */
    void*            out[3];  /* decoded (post-deblocking, post-SAO) planes Y, Cb, Cr; stride =
                                 plane width in samples; per component uint8_t samples at BitDepth
                                 8, uint16_t at 9..12.  NULL = do not download                  */
    void*            recon[3];/* optional in-loop-filter input (reconstruction before deblocking
                                 and SAO), same layout; NULL = skip.  Written by download, or
                                 read by upload with P265R_PIC_RECON_INPUT                     */
    uint16_t         pic_width;  /* this picture's size in luma samples; 0 = the context's      */
    uint16_t         pic_height; /* (p265r_params).  A batch may mix sizes up to the context's --
                                 the uneven tiles of one picture decoded as sub-pictures (the
                                 reference's column / row widths, pps.py:152-227) run in ONE
                                 launch.  Multiples of 8; the CTU records (PicSizeInCtbsY),
                                 planes, nofilter map and TB positions are of this size          */
    uint32_t         reserved;
} p265r_picture;

/* Sparse coefficients of one picture (parallel to pics[i]).  Entry = pos | (uint16_t)level << 16,
 * pos = y * N + x inside its TB (raster, N = 1 << log2_size), level the int16 TransCoeffLevel. */
typedef struct p265r_sparse_coef {
    const uint32_t* nz;
    uint64_t        n_nz;
} p265r_sparse_coef;

/* Per-phase device time of the last run, from HIP events on the context's stream. */
typedef struct p265r_timings {
    double   total_ms;        /* first kernel start -> last kernel end                     */
    double   residual_ms;     /* dequant + inverse transform kernels                       */
    double   intra_ms;        /* intra prediction + reconstruction (all wavefront steps)   */
    double   sao_ms;          /* in-loop filter kernel (deblocking + SAO)                  */
    int32_t  intra_launches;  /* kernel launches in the intra phase                        */
    int32_t  residual_launches;
    int32_t  sao_launches;
    int32_t  reserved;
} p265r_timings;

typedef struct p265r_ctx   p265r_ctx;
typedef struct p265r_batch p265r_batch;

/* Context on HIP device `device` for a sequence with parameters `params`. */
int  p265r_create(int device, const p265r_params* params, p265r_ctx** out);
void p265r_destroy(p265r_ctx* ctx);

/* Validate the records of n_pics pictures and copy them (plus output planes) into a
 * device-resident batch.  Synchronous w.r.t. the host buffers. */
int  p265r_batch_upload(p265r_ctx* ctx, const p265r_picture* pics, int n_pics, p265r_batch** out);
/* The same upload with the coefficients of the transformed blocks given as their non-zero levels
 * (opt-in; the dense call above stays the default).  sp[i] goes with pics[i].  A TB with P265R_TB_CBF
 * and neither P265R_TB_PCM nor P265R_TB_BYPASS (the transform classes and transform skip) is SPARSE:
 * its coef_off is the index of its first entry in sp[i].nz, its entry count the little-endian uint16
 * in reserved[0..1] (0 .. N*N; reserved[2] = 0), its entries contiguous with strictly increasing pos
 * (a level of 0 is allowed); positions not listed are 0.  PCM and bypass TBs keep the dense meaning:
 * coef_off into pics[i].coef (NULL / empty when the picture has none); every TB that is not sparse has
 * a count of 0.  Every record is checked on the host before anything reaches the device
 * (P265R_ERANGE: entries outside sp[i].nz, pos >= N*N; P265R_EINVAL: count > N*N, positions not
 * increasing, reserved[2] set, a count on a TB that is not sparse, sp or a needed nz NULL).  The
 * device expands the entries into the batch's coefficient pool at upload time: the batch is
 * afterwards the one the dense upload of the same coefficients gives, byte for byte, and runs the
 * same.  Uploads fewer bytes when few levels are non-zero (4 bytes per entry + 4 per sparse TB
 * against 2 per position).  No counterpart in the reference. */
int  p265r_batch_upload_sparse(p265r_ctx* ctx, const p265r_picture* pics, const p265r_sparse_coef* sp,
                               int n_pics, p265r_batch** out);
/* Host only (no context, no device): the sparse form of a dense picture.  tbs_out gets pic->n_tbs
 * records (sparse TBs: coef_off / count as above; PCM and bypass TBs: coef_off into raw_out, their
 * N*N samples compacted in TB order; reserved zeroed), nz_out the entries, raw_out the samples;
 * n_nz / n_raw get the counts.  With tbs_out, nz_out and raw_out all NULL only the counts are
 * returned; otherwise P265R_ERANGE when a capacity (nz_cap entries, raw_cap samples) is too small. */
int  p265r_sparsify(const p265r_picture* pic, p265r_tb* tbs_out, uint32_t* nz_out, uint64_t nz_cap,
                    uint64_t* n_nz, int16_t* raw_out, uint64_t raw_cap, uint64_t* n_raw);
/* Bytes of the host-to-device copies the batch's upload enqueued (dense or sparse: for comparing
 * the two).  No counterpart in the reference. */
int  p265r_batch_upload_bytes(p265r_ctx* ctx, p265r_batch* batch, uint64_t* h2d_bytes);
/* Enqueue reconstruction + SAO of every picture of the batch on the context stream. */
int  p265r_batch_run(p265r_ctx* ctx, p265r_batch* batch);
/* Wait for the batch and copy its planes into pics[i].out / pics[i].recon; returns what
 * p265r_batch_status returns afterwards. */
int  p265r_batch_download(p265r_ctx* ctx, p265r_batch* batch, const p265r_picture* pics, int n_pics);
/* Wait for every run enqueued on the batch's stream and report whether any run of the batch
 * since its upload failed on the device: P265R_OK, or P265R_EHIP when the intra row pipeline
 * gave up a (capped) dependency wait -- its output is then incomplete (p265r_last_hip_error
 * says which).  Lets a caller that re-runs a resident batch (a benchmark) check the work it
 * timed without downloading it.  No counterpart in the reference (which cannot fail this way). */
int  p265r_batch_status(p265r_ctx* ctx, p265r_batch* batch);
/* Per-picture digest of a batch's planes after every run enqueued on it, computed on the device
 * (no plane download): which = 0 the decoded (output) planes, 1 the reconstruction before the
 * in-loop filters.  out[3 * i + c] = sum over the 4-sample words of plane c of picture i (row y,
 * word k; the picture's own width W, W/4 words per row) of mix64(word | (y * W/4 + k) << 32)
 * mod 2^64, mix64 = the splitmix64 finalizer (p265_amd/digest.py restates it on the host);
 * n = 3 * the batch's pictures.  16-bit planes: words of 2 samples, W/2 per row -- in a wide context
 * (split_bit_depth) that holds for every plane, an 8-bit component included: the digest is of the
 * 16-bit device form (digest.plane_digest(..., wide=True)).  Returns what p265r_batch_status returns
 * afterwards.  Lets a benchmark check every picture it timed.  No counterpart in the reference. */
int  p265r_batch_digest(p265r_ctx* ctx, p265r_batch* batch, int which, uint64_t* out, int n);
/* The same digest ENQUEUED on the batch's lane after every run enqueued so far, into slot `slot`
 * (0 .. P265R_DIGEST_SLOTS-1) of the batch's digest buffer; returns without waiting (the buffer is
 * allocated at the first call).  p265r_batch_digest_slots waits for the lane and copies slots
 * [0, n_slots): out[(s * n_pics + i) * 3 + c].  Lets a caller check EVERY run of a pipelined schedule,
 * not only the last (a run's output is otherwise overwritten by the batch's next run).  A slot
 * written twice holds the later digest.  No counterpart in the reference. */
#define P265R_DIGEST_SLOTS 64
int  p265r_batch_digest_async(p265r_ctx* ctx, p265r_batch* batch, int which, int slot);
int  p265r_batch_digest_slots(p265r_ctx* ctx, p265r_batch* batch, uint64_t* out, int n_slots);
/* Intra jobs of the batch's last run (after job preparation: a 4x4 quad counts once, a Cb+Cr pair
 * once), luma and chroma, summed over its pictures; waits for the batch's lane.  For measurement
 * (bench.py: the row kernel's cycles per job).  No counterpart in the reference. */
int  p265r_batch_job_count(p265r_ctx* ctx, p265r_batch* batch, uint64_t* luma, uint64_t* chroma);
int  p265r_batch_free(p265r_ctx* ctx, p265r_batch* batch);

/* ---- device-side output: cropped frames in device memory, in the consumer's format ---------------
 * No counterpart in the reference (which parses the conformance window, sps.py:48-53, and never
 * applies it).  The arithmetic is fixed: B = BitDepth, crop origin (l, t).
 *   YUV formats: luma dst = src[t + y][l + x], chroma the same at half the coordinates; MSB16 shifts
 *     left by 16 - B; semi-planar plane 1 holds Cb at element 2 i and Cr at element 2 i + 1.
 *   Chroma at luma position (x, y) of the DECODED picture (indices clamped to that picture, not to
 *     the window): NEAREST C[y >> 1][x >> 1]; BILINEAR first vertically at scale 4, j = y >> 1:
 *     even y v[i] = C[j - 1][i] + 3 C[j][i], odd y v[i] = 3 C[j][i] + C[j + 1][i]; then, i = x >> 1:
 *     even x (v[i] + 2) >> 2, odd x (v[i] + v[i + 1] + 4) >> 3.
 *   RGB: D = 8 for P265R_SMP_U8, else B; y = Y - yoff, cb = Cb - half, cr = Cr - half;
 *     R = clip((cy y + crr cr + 8192) >> 14), G = clip((cy y - cgb cb - cgr cr + 8192) >> 14),
 *     B = clip((cy y + cbb cb + 8192) >> 14), int32, arithmetic shift, clip to 0 .. 2^D - 1, with the
 *     integers of p265r_export_coefficients.  F32 = float(v) * float(1 / (2^B - 1)) (one fp32
 *     multiply), F16 = that value rounded to nearest even. */
#define P265R_FMT_PLANAR      0u
#define P265R_FMT_SEMIPLANAR  1u
#define P265R_FMT_RGB_PLANAR  2u
#define P265R_FMT_RGB_PACKED  3u
#define P265R_SMP_NATIVE      0u
#define P265R_SMP_MSB16       1u
#define P265R_SMP_U8          2u
#define P265R_SMP_F16         3u
#define P265R_SMP_F32         4u
#define P265R_MAT_BT601       0u
#define P265R_MAT_BT709       1u
#define P265R_MAT_BT2020      2u
#define P265R_UP_NEAREST      0u
#define P265R_UP_BILINEAR     1u

typedef struct p265r_export_desc {
    uint32_t format;     /* P265R_FMT_PLANAR (Y, Cb, Cr planes) | P265R_FMT_SEMIPLANAR (Y, then CbCr
                            interleaved: NV12 / P010 / P012) | P265R_FMT_RGB_PLANAR (R, G, B planes:
                            "CHW") | P265R_FMT_RGB_PACKED (RGBRGB...: "HWC")                        */
    uint32_t sample;     /* P265R_SMP_NATIVE (uint8 at BitDepth 8, uint16 above, LSB-justified) |
                            P265R_SMP_MSB16 (uint16, v << (16 - BitDepth): P010 / P012; YUV formats
                            at BitDepth > 8 only) | P265R_SMP_U8 | P265R_SMP_F16 | P265R_SMP_F32
                            (the last three: RGB formats only)                                      */
    uint32_t matrix;     /* RGB only: P265R_MAT_BT601 | _BT709 | _BT2020 (non-constant luminance)  */
    uint32_t full_range; /* RGB only: 0 limited (16..235 / 16..240 scaled to BitDepth), 1 full     */
    uint32_t upsample;   /* RGB only: P265R_UP_NEAREST | P265R_UP_BILINEAR (chroma sited left /
                            vertically midway: chroma_sample_loc_type 0)                           */
    uint16_t crop_left, crop_right, crop_top, crop_bottom;   /* luma samples, even; per picture,
                            relative to THAT picture's size (ragged batches)                      */
    uint64_t plane_off[3]; /* byte offset of each destination plane inside a frame slot (semi-planar
                              uses 2, RGB packed 1); a multiple of the element size                */
    uint64_t pitch[3];     /* bytes between rows of each destination plane, >= the row's bytes     */
    uint64_t frame_bytes;  /* bytes between the frame slots of consecutive exported pictures       */
} p265r_export_desc;

/* host only, no context: fill plane_off / pitch / frame_bytes with the tight layout (planes back to
 * back, pitch = row bytes) of a w x h picture under desc's format / sample / crop; pitch_align > 1
 * rounds every pitch and plane offset up to it.  Validates the rest of desc. */
int  p265r_export_layout(const p265r_params* params, int pic_width, int pic_height,
                         p265r_export_desc* desc, uint32_t pitch_align);
/* host only: the eight integers of the RGB conversion, for desc at this bit depth:
 * {cy, crr, cgb, cgr, cbb, yoff, 1 << (B - 1), D} */
int  p265r_export_coefficients(const p265r_export_desc* desc, int bit_depth, int32_t out[8]);
/* enqueue, on the batch's lane and after every run enqueued on it so far, the conversion of pictures
 * pic_index[0..n) (NULL: all, in order) into frame slots 0..n) of dev_dst; returns without waiting
 * (p265r_batch_status / p265r_sync wait).  dev_dst is caller-owned device memory on the context's
 * device.  Everything is checked on the host before a kernel is launched: P265R_EINVAL for an unknown
 * enum value, a sample type that does not go with the format or bit depth, an odd crop, a crop that
 * leaves no sample of a listed picture, a pitch below the row bytes or no multiple of the element
 * size, planes of one slot that overlap, frame_bytes smaller than a slot, a pic_index entry outside
 * the batch or listed twice, a dev_dst that is not device memory of the context's device;
 * P265R_ERANGE when n slots do not fit in dst_bytes; P265R_ESTATE for a batch that was never run (a
 * P265R_PIC_RECON_INPUT batch whose filters never ran: it has no output planes yet).  n <= 65535.
 * Reads the planes p265r_batch_download returns; one kernel launch, no stream of its own. */
int  p265r_batch_export(p265r_ctx* ctx, p265r_batch* batch, const p265r_export_desc* desc,
                        void* dev_dst, uint64_t dst_bytes, const int32_t* pic_index, int n);

/* ---- scaled device-side output: every frame slot out_width x out_height -------------------------------------
 * No counterpart in the reference.  The SOURCE of a frame is the crop window of its picture (own size, as
 * above): W x H luma samples with origin (l, t); a chroma plane's window is W/2 x H/2 at (l/2, t/2).  Taps are
 * clamped to THE WINDOW, not to the decoded picture: a resized frame is a function of its window alone
 * (deliberately unlike P265R_UP_BILINEAR above, which reads decoded chroma outside the window).
 * desc->upsample is ignored: the filter decides how chroma is sampled.
 *
 * Per axis: n = luma window length, m = luma output length, step = floor((n << 16) / m).  An output sample sits
 * at half-sample coordinate h of the output LUMA grid, U(h) = (h * step) >> 1 its source position x 2^16 in luma
 * samples from the window's edge (h * step <= 2 n << 16: below 2^32, U below 2^31).
 *   output on the luma grid (Y planes; R, G, B), index i:       h = 2 i + 1 on both axes
 *   output on the chroma grid (planar / semi-planar Cb, Cr of a 4:2:0 source), index j:
 *                                                               h = 4 j + 1 horizontally, 4 j + 2 vertically
 *   (chroma_sample_loc_type 0: co-sited left, vertically midway).  n_p = n for a luma plane, n / 2 for chroma.
 * NEAREST   luma plane: index min(U >> 16, n - 1); chroma plane: min((U >> 16) >> 1, n / 2 - 1).  At m = n the
 *   result is byte-identical to p265r_batch_export with P265R_UP_NEAREST.
 * BILINEAR  pos = U - 32768 (luma plane); (U - 32768) >> 1 (chroma, horizontal); (U - 65536) >> 1 (chroma,
 *   vertical); arithmetic shifts; pos clamped to [0, (n_p - 1) << 16]; i0 = pos >> 16, i1 = min(i0 + 1, n_p - 1),
 *   f = (pos >> 8) & 255.  Value, int32, with a, b the taps i0, i1 of row i0 and c, d those of row i1:
 *     (((256 - fx) a + fx b) (256 - fy) + ((256 - fx) c + fx d) fy + 32768) >> 16.   Upscaling is legal.
 * AREA      exact box average, downscale only (m <= n on both axes).  In units of 1 / m of a luma sample,
 *   luma-grid output i covers [i n, (i + 1) n) and plane sample k covers [k e m, (k + 1) e m), e = 1 for luma and
 *   2 for chroma: chroma counts as two luma samples wide and high, its horizontal quarter-sample siting is
 *   ignored.  Chroma-grid outputs: the same with the plane's own n / 2, m / 2 and e = 1.  A sample's weight is
 *   the length of the overlap; the weights of one output sum to N, the covered length (n, or n / 2).
 *     value = (sum_y sum_x wy wx s + (Nx Ny >> 1)) / (Nx Ny), unsigned 64-bit, floor division.
 *   Windows of at most 8192 samples per axis (else P265R_EINVAL): the sum stays below 2^38, Nx Ny <= 2^26.
 * After the filter the planes are at output resolution and the arithmetic of p265r_batch_export applies unchanged
 * (MSB16 shift, CbCr interleave, the integer RGB conversion and clip, a monochrome source's R = G = B and grey
 * CbCr).  Float outputs: out = fl32(fl32(float(v) * scale[c]) + bias[c]), two separately rounded fp32 operations
 * (never one fma); F16 = that value rounded to nearest even.  Without P265R_RS_NORM scale[c] = float(1 / (2^B - 1))
 * and bias[c] = 0: the plain export's value. */
#define P265R_RS_NEAREST  0u
#define P265R_RS_BILINEAR 1u
#define P265R_RS_AREA     2u     /* exact box average; downscale only */
#define P265R_RS_NORM     1u     /* flags: scale[] / bias[] are used (F16 / F32 samples only) */

typedef struct p265r_resize_desc {
    uint32_t out_width, out_height;   /* 1 .. 16384; even for planar / semi-planar output of a 4:2:0 source
                                         and for semi-planar output of a monochrome source */
    uint32_t filter;                  /* P265R_RS_* */
    uint32_t flags;                   /* 0 | P265R_RS_NORM */
    float    scale[3], bias[3];       /* per output channel (R, G, B or Y, Cb, Cr order of the format) */
} p265r_resize_desc;

/* host only, no context: like p265r_export_layout, but the layout of an out_width x out_height frame (it does
 * not depend on a picture's size); validates desc and rs (P265R_EINVAL: an unknown filter or flag bit, a size of
 * 0 or above 16384, an odd size where the format has half-size chroma, P265R_RS_NORM with a sample type other
 * than F16 / F32, a non-finite scale or bias) */
int  p265r_resize_layout(const p265r_params* params, p265r_export_desc* desc, const p265r_resize_desc* rs,
                         uint32_t pitch_align);
/* host only: the source position of the output sample at half-sample coordinate h along one axis, as the kernels
 * compute it: n, m the luma window and output lengths, chroma = 1 for a chroma plane, vertical = 1 for the
 * vertical axis.  NEAREST: *i0 = *i1 = the index, *frac = 0; BILINEAR: i0, i1, f.  P265R_EINVAL for P265R_RS_AREA
 * (it has weights, not a position), n or m outside 1 .. 32767 / 16384, h outside 0 .. 2 m, an odd n with chroma. */
int  p265r_resize_position(uint32_t filter, int n, int m, int h, int chroma, int vertical,
                           int32_t* i0, int32_t* i1, int32_t* frac);
/* host only: the scalar reference of one plane through the arithmetic the kernels use (for tests).  src = the
 * plane's window origin (uint16 samples, stride samples between rows), nw x nh the LUMA window, mw x mh the LUMA
 * output size; chroma_plane: src is a chroma plane (nw / 2 x nh / 2); chroma_grid: the output is on the chroma grid
 * (mw / 2 x mh / 2, else mw x mh).  dst: the values, tight.  norm = {scale, bias} (or NULL): f32_out / f16_out
 * (each optional) get the float outputs of those values, fp16 as its 16 bits. */
int  p265r_resize_plane_host(const uint16_t* src, uint64_t stride, int nw, int nh, int chroma_plane, int chroma_grid,
                             uint32_t filter, int mw, int mh, int32_t* dst, const float* norm, float* f32_out,
                             uint16_t* f16_out);
/* as p265r_batch_export, every frame slot out_width x out_height: one kernel launch on the batch's lane, no
 * stream of its own, every check on the host before the launch.  The refusals of p265r_batch_export (the layout
 * is checked against the output size), those of p265r_resize_layout, and P265R_EINVAL for a crop window of ANY listed
 * picture above 32767 samples on an axis (every filter: the 32-bit position arithmetic), and for P265R_RS_AREA with an
 * output dimension larger than such a window or a window above 8192. */
int  p265r_batch_export_resized(p265r_ctx* ctx, p265r_batch* batch, const p265r_export_desc* desc,
                                const p265r_resize_desc* rs, void* dev_dst, uint64_t dst_bytes,
                                const int32_t* pic_index, int n);

/* ---- grid export: rows x cols pictures of a batch as ONE frame, cut to a window, turned and mirrored -----------
 * No counterpart in the reference.  What a HEIF `grid` item with `irot` / `imir` asks for (p265_amd/heif.py).
 *   Canvas.  All listed pictures have the same own size tw x th.  The canvas is cols tw x rows th luma samples; its
 *     luma sample (x, y) is sample (x % tw, y % th) of tile (y / th) * cols + x / tw; chroma the same at half sizes.
 *   Window.  [crop_left, out_width - crop_right) x [crop_top, out_height - crop_bottom) of the canvas, W x H.
 *   Frame F.  Exactly what p265r_batch_export would write if the canvas were one decoded picture of that size and
 *     the window its crop: sample types, the MSB16 shift, the CbCr interleave, the integer RGB conversion and the
 *     float scale carry over unchanged.  In particular the P265R_UP_BILINEAR chroma taps are clamped to the CANVAS
 *     (not to a tile, not to out_width x out_height) and cross tile seams.
 *   Orientation.  orientation = k | m << 2: the destination holds F turned k = 0..3 quarter turns ANTICLOCKWISE,
 *     then, with m = 1, mirrored left-right: numpy's np.rot90(F, k), then [:, ::-1].  Every plane is transformed
 *     alike; a CbCr pair or an RGB triple moves as one element.  Chroma is NOT re-sited after a turn: a chroma
 *     plane is turned as the array it is, so the half-sample offset of chroma_sample_loc_type 0 turns with it.
 *     With k odd the destination frame is H x W luma samples (planes of H/2 x W/2 chroma likewise), and
 *     p265r_grid_layout lays out that frame.
 *   Sources.  A monochrome context takes the monochrome rules of p265r_batch_export (Y; grey CbCr; R = G = B).
 *     rows = cols = 1 with orientation 0 is byte-identical to p265r_batch_export with the crop the window implies. */
typedef struct p265r_grid_desc {
    uint32_t rows, cols;            /* 1..256 each; rows * cols pictures per frame, row-major      */
    uint32_t out_width, out_height; /* the grid item's output size in luma samples                 */
    uint32_t orientation;           /* k | m << 2: k = 0..3 quarter turns ANTICLOCKWISE, then m = 1
                                       mirrors left-right.  Restated: np.rot90(F, k), then [:, ::-1] */
    uint32_t reserved[3];           /* 0, else P265R_EINVAL */
} p265r_grid_desc;

/* host only, no context: like p265r_export_layout, for the frame a grid of tile_width x tile_height pictures gives
 * under desc's format / sample / crop and grid's size and orientation; validates both (the P265R_EINVAL list of
 * p265r_batch_export_grid that needs no batch).  A canvas above 65535 samples on an axis is P265R_EINVAL. */
int  p265r_grid_layout(const p265r_params* params, int tile_width, int tile_height, const p265r_grid_desc* grid,
                       p265r_export_desc* desc, uint32_t pitch_align);
/* as p265r_batch_export: enqueued on the batch's lane behind its runs, no stream of its own, returns without
 * waiting, every check on the host before a launch.  ONE kernel launch for k even; for k odd two (the frame is
 * written untransposed into a staging area, then transposed through LDS), the staging allocated once per batch and
 * reused (grown only when a later call needs more).  pic_index lists rows * cols pictures per frame: tile
 * r * cols + c of frame f at f * rows * cols + r * cols + c; NULL = the batch in order (n_frames * rows * cols must
 * then equal the batch's pictures).  Every frame shares desc and grid.  P265R_EINVAL, on top of everything
 * p265r_batch_export refuses (desc's layout is checked against the ORIENTED frame): rows or cols 0 or above 256, an
 * orientation above 7, a reserved word set; listed pictures of differing own sizes; out_width outside
 * ((cols - 1) tw, cols tw] or out_height outside ((rows - 1) th, rows th]; an empty window; an odd window width or
 * height with a YUV format of a 4:2:0 source (odd is legal for RGB, and for a monochrome planar source); an odd
 * crop_left / crop_top on a 4:2:0 source (crop_right / crop_bottom only need to leave a legal window); a picture
 * listed twice; n_frames * rows * cols above 65535.  P265R_EUNSUPPORTED for a split_bit_depth context of unequal
 * depths. */
int  p265r_batch_export_grid(p265r_ctx* ctx, p265r_batch* batch, const p265r_export_desc* desc,
                             const p265r_grid_desc* grid, void* dev_dst, uint64_t dst_bytes, const int32_t* pic_index,
                             int n_frames);

/* ---- scaled grid export: every frame a grid of its own, every slot out_width x out_height ----------------------
 * No counterpart in the reference.  What a folder of HEIF photos asks for: grids of differing shape, window and
 * orientation into one dense batch.  For one frame, with rows x cols tiles of own size tw x th:
 *   Canvas and window.  As p265r_batch_export_grid defines them: the canvas is cols tw x rows th, the window
 *     [crop_left, out_width - crop_right) x [crop_top, out_height - crop_bottom) of it, W x H; here the crop is the
 *     FRAME's (p265r_grid_frame), and desc->crop_* must be 0.
 *   Pre-turn size.  With ow x oh = the resize descriptor's output size and orientation = k | m << 2:
 *     (pw, ph) = (ow, oh) for k even, (oh, ow) for k odd.
 *   R.  Exactly what p265r_batch_export_resized would write if the canvas were one decoded picture, the window its
 *     crop and the output size pw x ph: the step / U(h) positions, NEAREST, BILINEAR and AREA, the chroma siting, the
 *     MSB16 shift, the CbCr interleave, the integer RGB conversion and fl32(fl32(v scale) + bias) under P265R_RS_NORM
 *     carry over unchanged.  Taps are clamped to THE WINDOW: they cross tile seams inside it and never read outside it.
 *   Destination slot.  np.rot90(R, k), then [:, ::-1] when m is set.  Every plane is turned alike; a CbCr pair or an
 *     RGB triple moves as one element; chroma is NOT re-sited after a turn (the words of the grid export).
 *   Slot size.  Every slot is ow x oh, whatever its frame's grid, window or orientation; its layout is
 *     p265r_resize_layout's.
 *   Two identities, byte for byte: rows = cols = 1 with orientation 0 equals p265r_batch_export_resized with that
 *     crop; NEAREST with pw x ph = W x H equals p265r_batch_export_grid with P265R_UP_NEAREST.
 *   A chroma plane's window is W/2 x H/2 at (crop_left/2, crop_top/2): on a 4:2:0 source the window is even on both
 *     axes for EVERY format (an odd one would give the filters half a chroma sample, and break the second identity
 *     in the last column).  A monochrome source has no such limit except for semi-planar output. */
typedef struct p265r_grid_frame {      /* one frame of a ragged grid export */
    uint32_t rows, cols;               /* 1..256 */
    uint32_t out_width, out_height;    /* the grid item's size on ITS canvas */
    uint32_t crop_left, crop_right, crop_top, crop_bottom;   /* the window, per frame */
    uint32_t orientation;              /* k | m << 2 */
    uint32_t reserved[3];              /* 0 */
} p265r_grid_frame;

/* host only, no context: validates desc, rs and frames[0..n_frames) against a tile size (0: the params' size) as
 * p265r_batch_export_grid_resized does before it looks at a batch, and writes the constants its kernels use, twelve
 * int32 per frame: {first tile, cols, window left, top, W, H, pw, ph, reverse x, reverse y, transpose, index in the
 * staging area or -1}.  R is written reversed along x / y and then, for k odd, transposed:
 *   k = 0: (m, 0)   k = 2: (!m, 1)   k = 1: (1, m), transposed   k = 3: (0, !m), transposed */
int  p265r_grid_resize_plan(const p265r_params* params, int tile_width, int tile_height, const p265r_export_desc* desc,
                            const p265r_resize_desc* rs, const p265r_grid_frame* frames, int n_frames, int32_t* out);
/* as p265r_batch_export_grid and p265r_batch_export_resized: enqueued on the batch's lane behind its runs, no stream
 * of its own, returns without waiting, every check on the host before a launch.  At most TWO kernel launches whatever
 * the mix of orientations: frames with k even are written straight to their slot; frames with k odd go through the
 * grid export's staging area (allocated once per batch, reused, grown only when needed) and one transpose launch.
 * pic_index lists the tiles frame after frame: frame f's tiles start at the sum of rows * cols of the frames before
 * it; NULL = the batch in order (the sum over all frames must then equal the batch's pictures).
 * P265R_EINVAL: everything p265r_batch_export_resized and p265r_batch_export_grid refuse, applied per frame (listed
 * pictures of differing own sizes across the whole call included); desc->crop_* non-zero; a window above 32767 on an
 * axis; P265R_RS_AREA with pw > W or ph > H, or with a window above 8192 on an axis; an odd window on a 4:2:0
 * source; n_frames or the tiles listed above 65535.  P265R_EUNSUPPORTED for a context of unequal depths.  Monochrome
 * contexts follow the monochrome rules of the two existing exports. */
int  p265r_batch_export_grid_resized(p265r_ctx* ctx, p265r_batch* batch, const p265r_export_desc* desc,
                                     const p265r_resize_desc* rs, const p265r_grid_frame* frames, int n_frames,
                                     void* dev_dst, uint64_t dst_bytes, const int32_t* pic_index);

/* ---- device-side picture hash: the decoded_picture_hash SEI values (D.3.19) computed in device memory ----
 * No counterpart in the reference (no SEI support, nalu.py:130-131).  The hash of a plane runs over its
 * pictureData: the samples of the picture's OWN size (uncropped) in raster order, one byte per sample at
 * BitDepth 8, two (little-endian) above.  The 16 bytes per plane have the form the SEI carries (and
 * p265fe_plane_hash writes): MD5 16 bytes; CRC 2 bytes big-endian, the rest 0; checksum 4 bytes big-endian,
 * the rest 0.  The values equal P265FE_HASH_*. */
#define P265R_HASH_MD5      0
#define P265R_HASH_CRC      1
#define P265R_HASH_CHECKSUM 2
/* enqueue, on the batch's lane and after every run and export enqueued on it so far, the hash of the planes
 * p265r_batch_download returns, into a per-batch buffer of 16 bytes per plane (allocated at the first call,
 * freed with the batch; a later call overwrites it); returns without waiting.  P265R_EINVAL for a NULL
 * pointer or an unknown type, P265R_ESTATE for a batch that was never run; checked before any launch. */
int  p265r_batch_hash_async(p265r_ctx* ctx, p265r_batch* batch, int hash_type);
/* wait for the batch's lane and copy the buffer: out[(3 * i + c) * 16 ..], n_bytes = 48 * n_pics
 * (else P265R_EINVAL); P265R_ESTATE before any p265r_batch_hash_async.  Returns what p265r_batch_status
 * returns. */
int  p265r_batch_hash_read(p265r_ctx* ctx, p265r_batch* batch, uint8_t* out, int n_bytes);
/* host only, no context: the same hash of a host plane of width x height samples of bytes_per_sample (1, 2)
 * bytes, rows stride_bytes apart, through the arithmetic the kernels use: the message is cut into segments of
 * seg_words 32-bit words (0: one segment) whose terms are combined last segment first (MD5, a serial chain,
 * ignores the cut).  P265R_EINVAL: a NULL pointer, a non-positive size, a width or height that is no
 * multiple of 4, bytes_per_sample not 1 or 2, a stride below the row's bytes, an unknown type, a plane of
 * 2^29 bytes or more. */
int  p265r_plane_hash_host(const void* plane, int width, int height, uint64_t stride_bytes,
                           int bytes_per_sample, int hash_type, uint32_t seg_words, uint8_t out[16]);

/* Convenience: upload + run (asynchronous) ... */
int  p265r_submit(p265r_ctx* ctx, const p265r_picture* pics, int n_pics);
/* ... then block until outputs are written into the pictures given to submit. */
int  p265r_wait(p265r_ctx* ctx);

/* Block until the context's streams are idle. */
int  p265r_sync(p265r_ctx* ctx);
/* Batch pipelining (no counterpart in the reference; a throughput knob of this back-end):
 * batches uploaded afterwards are bound round-robin to `depth` (1..16) HIP streams, so the
 * residual and loop-filter phases of one batch run beside the intra phase of another (small
 * batches: whole batches side by side).  Every stream wants a hardware queue of its own: HIP's
 * default GPU_MAX_HW_QUEUES=4 serves depth <= 3 (+ the upload stream); set GPU_MAX_HW_QUEUES >=
 * depth + 1 before the process first touches HIP for deeper pipelines (min(32, 2 x depth + 2) for
 * batches of >= one picture per CU, whose prep / residual phases get streams of their own; the
 * runtime accepts at most 32, so past depth 15 such batches share hardware queues).
 * Runs of one batch stay ordered; p265r_sync waits for every stream.  Default 1. */
int  p265r_set_pipeline(p265r_ctx* ctx, int depth);
/* Scaling lists (scaling_list_enabled = 1; decoder/scaling.py:32-44, m[x][y] = ScalingFactor[sizeId]
 * [matrixId][x][y]): the intra ScalingFactor arrays, 2032 bytes, each matrix row-major m[y][x] (y the
 * row): 4x4 Y, Cb, Cr at byte 0, 16, 32; 8x8 Y, Cb, Cr at 48, 112, 176; 16x16 Y, Cb, Cr at 240, 496,
 * 752 (DC included); 32x32 Y at 1008 -- the derivation of 7.4.5 from the SPS / PPS scaling_list_data
 * (default lists included) is the caller's (libp265fe.so delivers it with every picture).  Values
 * 1..255.  Applies to every later run of the context (waits for the runs in flight first); a context
 * with scaling_list_enabled refuses to run (P265R_ESTATE) until it is set. */
#define P265R_SCALING_FACTOR_BYTES 2032
int  p265r_set_scaling_factors(p265r_ctx* ctx, const uint8_t* factors, int n_bytes);
/* Measurement knob (no counterpart in the reference): force the intra row kernel's build for this
 * context's later runs -- 8 or 12 waves per workgroup -- or 0 (default) to pick it per run (12 for a
 * batch alone, 8 beside other lanes' runs, the latency layouts for small batches).  Lets a benchmark
 * time the build its pipelined steps run, in isolation. */
int  p265r_set_row_waves(p265r_ctx* ctx, int waves);
/* Enable (1, which also starts a new accumulation) / disable (0) per-phase HIP-event
 * timing of every p265r_batch_run; read the last run's timings, or the sums over all runs
 * since enabling (runs may be queued back to back: nothing here waits per run). */
int  p265r_set_timing(p265r_ctx* ctx, int enable);
int  p265r_last_timings(p265r_ctx* ctx, p265r_timings* out);
int  p265r_timings_total(p265r_ctx* ctx, p265r_timings* out, int* n_runs);

/* Effective configuration of a context as a JSON object (intra schedule, waves per workgroup,
 * loop-filter kernel choice, pipeline depth, and which P265R_* environment knobs overrode the
 * defaults): writes at most size-1 bytes + NUL into buf, returns the full length (like snprintf)
 * or an error code.  Lets a benchmark record what it measured. */
int  p265r_describe(p265r_ctx* ctx, char* buf, int size);

/* Number of HIP devices visible (>= 0), or an error code. */
int  p265r_device_count(void);
const char* p265r_strerror(int code);
/* Text of the last HIP error seen by this library (thread-local), "" if none. */
const char* p265r_last_hip_error(void);
/* Library ABI version (P265R_ABI_VERSION). */
uint32_t p265r_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* P265R_H */
