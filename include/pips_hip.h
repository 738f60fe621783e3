/*
 * pips_hip.h -- C ABI of libpips_hip.so: the PIPs particle-tracker inference hot path
 * (reference: aharley/pips  nets/pips.py:428-611, Pips.forward) as hand-written HIP for
 * gfx950 (MI355X / CDNA4).
 *
 * The reference has no FFI of its own: the operator API of the path is the Python class
 * nets.pips.Pips (nets/pips.py:400-611).  The replacement keeps that class
 * (pips_amd.Pips) and puts ALL arithmetic behind the entry points below; each one names
 * the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PIPS_E_* code; the text of the
 *     last error of the calling thread is available from pips_last_error();
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - the caller owns every buffer (inputs, outputs, weight arena, workspace); the
 *     library never allocates, frees or synchronises (the *_timed entry points excepted).  The
 *     only state kept between calls is idempotent: the dynamic-LDS attribute of each kernel
 *     instantiation (raised on its first launch on a device, tracked per device with atomics)
 *     and the device's compute-unit count (one atomic slot per device).  The library reads no
 *     environment variables (the PIPS_* tuning hooks exist only in a -DPIPS_TUNING build,
 *     pips_amd/_build.py --tuning, where each is read once in a thread-safe static initialiser).
 *     Calls are re-entrant and stream-ordered
 *     on `stream` (a hipStream_t passed as void*).  hipGraph capture: run the same call once
 *     eagerly first (so no attribute is set while capturing), then capture and replay -- replays
 *     are bit-identical to the eager call (tests/test_forward_gpu.py::test_forward_in_hip_graph);
 *   - all tensors are dense fp32 unless stated; "frames" F = B*S; mixer rows are ordered
 *     m = (b*N + n)*S + s ("particle-major"), map levels are channel-last
 *     [F][H_l][W_l][128].
 */
#ifndef PIPS_HIP_H
#define PIPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIPS_OK            0
#define PIPS_E_ARG        -1   /* bad shape / null pointer / unsupported size        */
#define PIPS_E_WORKSPACE  -2   /* workspace too small                                */
#define PIPS_E_LAUNCH     -3   /* hipLaunch error (see pips_last_error)              */

#define PIPS_S        8        /* frames per window of the shipped checkpoints; other S: the _s entry points */
#define PIPS_C        128      /* latent channels            nets/pips.py:408        */
#define PIPS_LEVELS   4        /* correlation pyramid levels nets/pips.py:409        */
#define PIPS_RADIUS   3        /* correlation radius         nets/pips.py:410        */
#define PIPS_NCORR    196      /* LEVELS * (2R+1)^2                                  */
#define PIPS_KIN      519      /* mixer input width          nets/pips.py:289        */
#define PIPS_KIN_PAD  544      /* same, zero-padded to a multiple of 32              */
#define PIPS_DMIX     512      /* mixer width                nets/pips.py:298        */
#define PIPS_DEPTH    12       /* mixer depth                nets/pips.py:300        */
#define PIPS_NOUT     1040     /* S*(C+2)                    nets/pips.py:299        */
#define PIPS_NPARAMS  200      /* tensors in the reference state dict                */

/* flags of pips_forward / pips_track */
#define PIPS_FLAG_REUSE_MAPS  1   /* pips_forward: skip the encoder, the workspace already holds the maps (of a call with the
                                     same B,S,H,W,stride AND the same encoder flags: they describe the maps) */
#define PIPS_FLAG_BF16_ENCODER 4  /* the encoder the way torch.autocast(bfloat16) runs it: bf16 MFMA operands in all 22
                                     convolutions (7x7 stem included) and bf16 activation maps between the layers;
                                     statistics from the fp32 accumulators, normalisation / ReLU / adds / resizes in
                                     fp32 arithmetic rounded once on store; the pyramid handed to the tracker is fp32 */
#define PIPS_FLAG_RGB_U8      8   /* rgbs points at uint8 (B,S,3,H,W) frames instead of float: same values, a
                                     quarter of the input bytes (the decoded frames of demo.py:136-144) */
#define PIPS_FLAG_BF16_MIXER  2   /* bf16 MFMA operands in the channel-mix and head Linear layers (BASELINE
                                     config 3); accumulation, norms, GELU, residual stream, gather stay fp32 */

#define PIPS_FLAG_BF16_STREAM 64  /* with PIPS_FLAG_BF16_MIXER (window length 8): the mixer's residual stream is a bf16 tensor, as
                                     PreNormResidual's `fn(norm(x)) + x` is under autocast (nets/pips.py:93-100: both terms bf16) --
                                     token mixing and the down-projections read it, add in fp32 and round once on the way out;
                                     LayerNorm statistics, GELU and accumulation stay fp32.  IGNORED for window lengths other than
                                     8 (the generic-S token mixing keeps an fp32 stream).  pips_amd.Pips sets it by default with a
                                     bf16 mixer since round 5 (outputs differ from rounds 1-4 by ~1e-2 px at BASELINE configs[2];
                                     Pips.mixer_stream_dtype = torch.float32 restores the fp32 stream) */
#define PIPS_FLAG_BF16_MAPS   32  /* pips_track / pips_mixer_input_build_ex: the correlation gather reads the bf16 MIRROR of the
                                     pyramid (behind the fp32 levels, pips_pyramid_mirror_offset; written by the bf16 encoder or
                                     pips_pyramid_mirror) -- the reference's rounding point under autocast, where the encoder's
                                     output is a bf16 tensor; pips_forward sets it itself when both BF16 flags are given */
#define PIPS_FLAG_SPLIT_BF16  16  /* fp32-grade "split-bf16" matrix path: every fp32 operand is split exactly into
                                     three bf16 terms (round-to-nearest at each step), six exact bf16 products per fp32 product, fp32 accumulation
                                     (pips_gemm_f32x3) -- all mixer Linear layers and the convolutions where it is
                                     faster; same accuracy class as the exact-fp32 MFMA path, not bitwise equal to
                                     it; takes precedence over the two BF16 flags */

const char* pips_last_error(void);
/* 3 (round 6).  History: 2 -> 3 (buffer contracts that grew in round 5; a caller holding buffers sized by the v2 rules gets
 * out-of-range reads on a dense query set with PIPS_FLAG_BF16_MAPS): pips_pyramid_floats() includes a SLACK behind the bf16 mirror
 * (4 rows + 16 pixels of the coarsest level: gather_mfma_kernel fetches whole 8 x 4 pixel blocks unmasked past the last level's
 * last frame), and the tiled gather's scratch (inside pips_track_workspace_bytes* / pips_workspace_bytes) carries the slot map,
 * the bf16 feature rows of the sorted order and a batch of slots of slack -- size every buffer with the query functions of THIS
 * version; PIPS_EPI_RES_BF16 is a public constant; pips_mixer_gemm_train honours PIPS_FLAG_BF16_STREAM.
 * 1 -> 2: the pyramid buffer of EVERY encoder mode is pips_pyramid_floats() long (the bf16 encoder writes
 * a bf16 mirror of the four levels behind them, at pips_pyramid_mirror_offset -- a buffer sized from the level offsets alone
 * is too short); the PIPS_PACK_FFN arena section and pips_mixer_fwd_bf16_fused (round 3's fused FeedForward, measured slower than
 * the two GEMMs again in round 4 -- tools/experiments/) are gone.
 * Still 3 after additions that change no existing entry point: pips_track_win and pips_mixer_input_build_win (per-particle
 * time direction win_dir); pips_track_ring, pips_mixer_input_build_ring and pips_pyramid_append (a ring of R frame slots
 * for streamed video); pips_chain_hop, pips_chain_gather, pips_chain_step, pips_chain_workspace_bytes and pips_chain_threshold
 * (the visibility-aware chaining of chain_demo.py:40-83, one call per hop); pips_track_clips, pips_mixer_input_build_clips,
 * pips_chain_hop_clips, pips_chain_gather_clips and pips_chain_step_clips (the windows of several videos on one flat cache:
 * a per-particle video index).  pips_chain_workspace_bytes grew by the staged video indices: size with THIS library.
 * pips_stream_select, pips_stream_round, pips_stream_emit and pips_stream_workspace_bytes (the rounds of a streamed video: which
 * queries are ready, which join, one hop, which frames are final -- one call per round); pips_track_rings,
 * pips_mixer_input_build_rings, pips_pyramid_append_at, pips_stream_select_clips, pips_stream_round_clips,
 * pips_stream_workspace_bytes_clips and pips_stream_emit_cols (several streamed videos on one flat cache of rings: one state and
 * one round for all of them); pips_stream_keep (queries leave a running stream: the kept columns of the state in narrower
 * arrays); pips_cover_step and pips_cover_workspace_bytes (which queries of a stream are retired and where new ones are seeded, so
 * that a bounded set of tracks stays spread over the frame); pips_corner_table and pips_cover_place (the best corner of each
 * cover cell of each frame, and the seeds of a cover step moved from the cell centres onto them); pips_cover_step_thin and
 * pips_cover_thin_workspace_bytes (the cover step with at most per_cell tracks in a cell: the youngest surplus are retired);
 * pips_cut_table and pips_cut_workspace_bytes (the regional luma histogram of each raw frame and its distance to the frame before:
 * where a video has its scene cuts); pips_frames_import (a decoder's NV12, I420 or packed RGB frames, pitched, to the planar frames
 * every entry point reads, resized in the same pass); pips_frames_import_ex (the same with a filter argument -- the antialiasing
 * triangle filter beside the two-tap bilinear -- and the 10-bit formats P010 and I010); pips_tracks_draw and
 * pips_draw_workspace_bytes (the trails of the tracks drawn onto the decoder's 8-bit surfaces, in place);
 * pips_conv_nhwc_f32_r and pips_encoder_l1_fused (the LDS-resident 64 -> 64 convolution of the fp32 encoder's layer 1 and whether
 * the encoder takes it); pips_inorm_apply_f32 (pips_inorm_apply on fp32 maps with mode 3 beside modes 0..2);
 * pips_tracks_draw_ex (pips_tracks_draw with the 10-bit surfaces P010 and I010 and a fade table: trails whose opacity falls with
 * age; pips_draw_workspace_bytes sizes both at the same figure); pips_motion_fit and pips_motion_workspace_bytes (the camera motion
 * between consecutive rows of a trajectory tensor: an exact consensus similarity); pips_frames_warp (the decoder's surfaces
 * resampled through a per-frame affine map in exact integers: frames out, stabilised); pips_motion_layers and
 * pips_motion_layers_workspace_bytes (the consensus of pips_motion_fit peeled into up to 8 motion layers a pair, with the overlap
 * table that links a pair's layers to those of the pair before: what moves, beside the camera); pips_frames_warp_fill
 * (pips_frames_warp with a list of candidate source frames per output frame: the border of a stabilised frame filled from its
 * neighbours). */
int         pips_abi_version(void);

/* ---- weights ------------------------------------------------------------------------
 * Replaces: nn.Module parameter storage + load_state_dict (saverloader.py:58-59).
 * `params[i]` is the device pointer of the i-th tensor of the reference state dict in
 * its canonical order (nets/pips.py:400-426; pips_amd/weights.py:param_table), in the
 * reference's own layout.  The arena receives the kernel-side layouts
 * (conv [Cout][kh][kw][Cin], stem [ci*kh*kw][64], first Linear zero-padded to 544
 * columns, updater Linear transposed, the rest verbatim). */
size_t pips_weight_arena_bytes(void);
int    pips_repack_weights(const void* const* params_host, int nparams, void* arena, void* stream);
/* The arena's three sections can be (re)built separately: PIPS_PACK_FP32 (the fp32 layouts, from params), PIPS_PACK_BF16
 * (bf16 copies of every matrix-core weight: the bf16-operand modes) and PIPS_PACK_SPLIT (three bf16 planes per weight: the
 * split-bf16 mode) -- the last two are derived from the arena's fp32 section (params may be null without PIPS_PACK_FP32),
 * so a process packs only what its matrix mode reads.  pips_repack_weights = all sections. */
#define PIPS_PACK_FP32  1
#define PIPS_PACK_BF16  2
#define PIPS_PACK_SPLIT 4
int    pips_repack_weights_ex(const void* const* params_host, int nparams, void* arena, int sections, void* stream);

/* ---- any window length: Pips(S != 8) ----------------------------------------------------
 * Replaces: the S argument of nets.pips.Pips.__init__ (nets/pips.py:401-402), which sizes the token-mixing weights
 * (4S x S, S x 4S: :102-109,117) and the head (S*(C+2) x 512: :295-301).  Every entry point above and below without an S
 * argument means S = PIPS_S = 8, the window of every shipped checkpoint, and runs kernels specialised for it; the _s
 * variants take 1 <= S <= PIPS_S_MAX (the arena must have been packed for the same S) and run the token mixing, the final
 * LayerNorm + mean and the state update on generic kernels (same arithmetic, not tuned), the GEMMs and the gather on
 * the same kernels as S = 8.  pips_forward / pips_workspace_bytes take S from their own argument.  Rows of the mixer output
 * (delta) are pips_delta_stride(S) = S*(C+2) rounded up to a multiple of 4 floats apart.  (Round 6: 32, was 16 -- the generic
 * kernels are instantiated for 16 and for 32 token registers and picked by S.) */
#define PIPS_S_MAX 32
size_t pips_weight_arena_bytes_s(int S);
int    pips_repack_weights_s(const void* const* params_host, int nparams, void* arena, int S, int sections, void* stream);
int    pips_delta_stride(int S);
size_t pips_mixer_workspace_bytes_s(int M, int S);
int    pips_mixer_fwd_s(const void* arena, const float* X, int M, int S, int flags, float* delta,
                        void* workspace, size_t workspace_bytes, void* stream);     /* flags: BF16_MIXER (+ BF16_STREAM at S = 8) / SPLIT_BF16 */
size_t pips_track_workspace_bytes_s(int B, int N, int S);
/* pips_track / pips_track_ce (below) with the window length as an argument; ce_* may be NULL */
int    pips_track_s(const void* arena, const float* pyramid, int B, int T, int H8, int W8, const float* xys,
                    const float* coords_init, const float* feat_init, const int* win_start, const float* times, int N,
                    int stride, int iters, int flags, int S, void* workspace, size_t workspace_bytes, float* out_trajs,
                    float* out_vis, float* out_ffeat0, const float* ce_tgt, float* ce_terms, void* ce_ws,
                    size_t ce_ws_bytes, void* stream);

/* ---- whole forward -------------------------------------------------------------------
 * Replaces: Pips.forward, inference branch (nets/pips.py:428-611 minus the dead fcp
 * upsample :504-511, the sw visualisation branches and the losses :600-606).
 *   rgbs        (B,S,3,H,W) fp32 0..255, NCHW exactly as callers pass it (demo.py:40)
 *   xys         (B,N,2) pixels
 *   coords_init (B,S,N,2) pixels or NULL   (nets/pips.py:452-455)
 *   feat_init   (B,N,128) or NULL          (nets/pips.py:461-465)
 *   times       (S) = torch.linspace(0,S,S) (nets/pips.py:519)
 *   out_trajs   (iters+1,B,S,N,2) pixels: entry 0 = initial coords*stride
 *               (coord_predictions2[0]), entries 1.. = coord_predictions
 *   out_vis     (B,S,N) logits             (nets/pips.py:559)
 *   out_ffeat0  (B,N,128) initial feature  (nets/pips.py:463, returned when return_feat)
 * stride is 4 or 8 in the reference's callers; any value >= 1 whose map H/stride x W/stride is at least 16 x 16.
 * THE MAP SIZE RULE, shared by every entry point that samples correlation windows (pips_forward*, pips_track* in all its forms,
 * pips_mixer_input_build* in all its forms, pips_chain_hop*, pips_stream_round*): the sampler normalises the coordinates of a
 * level with 2 x / (W - 1) - 1 (nets/pips.py:318-319), so a pyramid level one pixel wide or high divides by zero and makes
 * every position behind the query frame NaN.  All four levels must be at least 2 x 2: H8 >= 16 and W8 >= 16 (frames of at least
 * 128 px a side at stride 8, 64 px at stride 4).  A smaller map is PIPS_E_ARG ahead of any launch -- no output or workspace byte
 * is written, the encoder is not run -- and pips_last_error() names the map.  The encoder, the pyramid copies, the sizing
 * queries and pips_score_map_prepare divide by no size - 1 and keep taking maps down to 8 x 8.
 * flags: PIPS_FLAG_REUSE_MAPS = skip the encoder and reuse the pyramid already in the workspace
 *        (same B,S,H,W,stride as the call that produced it); PIPS_FLAG_BF16_MIXER. */
size_t pips_workspace_bytes(int B, int S, int H, int W, int N, int stride);
int    pips_forward(const void* arena, const float* rgbs, const float* xys,
                    const float* coords_init, const float* feat_init, const float* times,
                    int B, int S, int H, int W, int N, int stride, int iters, int flags,
                    void* workspace, size_t workspace_bytes,
                    float* out_trajs, float* out_vis, float* out_ffeat0, void* stream);

/* ---- tracker on cached maps ------------------------------------------------------------
 * Replaces: Pips.forward minus the encoder, for callers that re-run the tracker on maps they
 * already have: the dense-grid loop of test_on_davis.py:103-130 (one encoder pass, many query
 * chunks) and the visibility-aware chaining of chain_demo.py:40-83 / test_on_badja.py:64-112
 * (one encoder pass per video frame instead of per particle and hop).
 *   pyramid    packed 4-level channel-last maps of B clips x T frames (pips_encoder_fwd with
 *              F = B*T; per-frame InstanceNorm makes a frame's maps independent of its clip)
 *   win_start  (B*N) int32 first frame of each particle's 8-frame window, or NULL (= 0);
 *              frames past T-1 repeat frame T-1 (chain_demo.py:50-52)
 *   win_dir    (pips_track_win only) (B*N) int32 time direction of each particle's window, or NULL (= all forward);
 *              only the sign is used: < 0 = backward.  Row s of a backward window reads frame
 *              clamp(win_start - s, 0, T-1): frames before 0 repeat frame 0, which is chain_demo.py's loop run on the
 *              time-reversed video.  The time embedding is still s and row 0 (the query frame) still locks the start.
 *              Needs win_start; windowed particles always take the direct gather.
 * All other arguments as pips_forward.  T = 8 and win_start = NULL is exactly the forward.  H8, W8 >= 16 (the map size rule at
 * pips_forward); a smaller map is PIPS_E_ARG ahead of any launch. */
size_t pips_track_workspace_bytes(int B, int N);
int    pips_track(const void* arena, const float* pyramid, int B, int T, int H8, int W8,
                  const float* xys, const float* coords_init, const float* feat_init,
                  const int* win_start, const float* times, int N, int stride, int iters, int flags,
                  void* workspace, size_t workspace_bytes,
                  float* out_trajs, float* out_vis, float* out_ffeat0, void* stream);
/* pips_track_s plus win_dir (see above), without the score-map terms; win_dir = NULL is exactly pips_track_s */
int    pips_track_win(const void* arena, const float* pyramid, int B, int T, int H8, int W8,
                      const float* xys, const float* coords_init, const float* feat_init,
                      const int* win_start, const int* win_dir, const float* times, int N, int stride, int iters,
                      int flags, int S, void* workspace, size_t workspace_bytes,
                      float* out_trajs, float* out_vis, float* out_ffeat0, void* stream);
/* pips_track_win on a ring of R frame slots per clip (streamed video, pips_pyramid_append): the pyramid is laid out for R
 * frames (pips_pyramid_floats(B*R, ...)), T is the number of logical frames appended so far and only the clamp bound, and
 * logical frame f lives in slot f mod R.  Row s of a window reads slot clamp(win_start + dir*s, 0, T-1) mod R; the point
 * sample of feat_init = NULL reads slot clamp(win_start, 0, T-1) mod R.  R = T is exactly pips_track_win.  The caller
 * keeps every frame a window can read in the ring: with T frames appended, frames T-R .. T-1. */
int    pips_track_ring(const void* arena, const float* pyramid, int B, int T, int R, int H8, int W8,
                       const float* xys, const float* coords_init, const float* feat_init,
                       const int* win_start, const int* win_dir, const float* times, int N, int stride, int iters,
                       int flags, int S, void* workspace, size_t workspace_bytes,
                       float* out_trajs, float* out_vis, float* out_ffeat0, void* stream);
/* Several videos in one call.  The pyramid is ONE flat linear cache (B = 1, R = T) whose frame axis holds the frames of V
 * videos of the same frame size one after the other, T = the sum of their lengths, each video's frames encoded as if alone:
 *   clip_first  (V) device int32: first flat frame of video v
 *   clip_frames (V) device int32: frames of video v
 *   win_clip    (N) device int32: the video of each particle, or NULL
 * Row s of particle n's window reads flat frame clip_first[v] + clamp(win_start + dir*s, 0, clip_frames[v]-1), v = win_clip[n]:
 * win_start counts frames of the particle's OWN video, and the repeats past its last frame and before its frame 0 stop at
 * that video, never at a neighbour's.  The point sample of feat_init = NULL reads row 0's frame.  Results per particle are what
 * pips_track_win gives on that video's own cache (bit for bit while the mixer's GEMMs take the same route at both row counts).
 * Containment: v is clamped to [0, V-1] and the flat frame to [0, T-1] -- a corrupt index reads a wrong frame, never outside
 * the buffer.  Windowed particles take the direct gather.  win_clip = NULL: exactly pips_track_ring plus the score-map block of
 * pips_track_s (V and the tables are not read).  With win_clip, PIPS_E_ARG ahead of any launch for: V < 1, a NULL clip_first /
 * clip_frames, a NULL win_start, B != 1, R != T, a non-NULL ce_tgt. */
int    pips_track_clips(const void* arena, const float* pyramid, int B, int T, int R, int H8, int W8,
                        const float* xys, const float* coords_init, const float* feat_init,
                        const int* win_start, const int* win_dir,
                        const int* win_clip, const int* clip_first, const int* clip_frames, int V,
                        const float* times, int N, int stride, int iters, int flags, int S,
                        void* workspace, size_t workspace_bytes,
                        float* out_trajs, float* out_vis, float* out_ffeat0,
                        const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes, void* stream);
/* Several STREAMED videos in one call: the flat cache holds V rings of R frame slots each (R is one value per cache) instead of
 * V linear videos.  The arguments are those of pips_track_clips with F in the place of T -- the pyramid is laid out for F frame
 * slots (pips_pyramid_floats(F, ...)), F >= V*R -- and R = the slots of each video's ring:
 *   clip_first  (V) device int32: first flat slot of video v's ring (v*R for rings laid side by side)
 *   clip_frames (V) device int32: logical frames appended to video v so far; may exceed R; the caller updates it as it appends
 *                                 (pips_pyramid_append_at)
 * Row s of particle n's window reads flat slot clip_first[v] + (clamp(win_start + dir*s, 0, clip_frames[v]-1) mod R), v =
 * win_clip[n]; the caller keeps every frame a window can read in its ring (pips_track_ring's rule, per video).  Containment as
 * for pips_track_clips: v is clamped to [0, V-1], the flat slot to [0, F-1].  Results per particle are what pips_track_ring gives
 * on that video's own ring (bit for bit while the mixer's GEMMs take the same route at both row counts).  PIPS_E_ARG ahead of any
 * launch for: V < 1, R < 1, a NULL win_clip / clip_first / clip_frames / win_start, B != 1, F < V*R, a non-NULL ce_tgt. */
int    pips_track_rings(const void* arena, const float* pyramid, int B, int F, int R, int H8, int W8,
                        const float* xys, const float* coords_init, const float* feat_init,
                        const int* win_start, const int* win_dir,
                        const int* win_clip, const int* clip_first, const int* clip_frames, int V,
                        const float* times, int N, int stride, int iters, int flags, int S,
                        void* workspace, size_t workspace_bytes,
                        float* out_trajs, float* out_vis, float* out_ffeat0,
                        const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes, void* stream);

/* ---- visibility-aware chaining: one call per hop ----------------------------------------
 * Replaces: the hop loop body of chain_demo.py:40-83 (test_on_badja.py:64-112) for a whole set of particles -- read the
 * start position at the window start (:47), run the model on the 8-frame window (:54-57, features carried from the first
 * window), write the window into the trajectory (:59-61), scan frames 7..2 for the latest one whose sigmoid visibility
 * beats the threshold 0.9, lowered by 0.02 whenever the scan reaches frame 1 (:63-77), advance the window start by that step
 * (:79) -- and the bookkeeping of which particles are still inside the video.  Window length 8 only (the scan is written for it).
 *
 * The caller owns the state, all of it on the device:
 *   trajs   float (L,n,2)  trajectories; logical frame f lives in row ((f + base) mod L + L) mod L
 *   vis     float (L,n)    visibility logits, same rows; may be NULL
 *   cur     int32 (n)      window start of each particle (logical frame)
 *   dir     int32 (n)      time direction, only the sign is used (< 0: backward, pips_track_win's win_dir); NULL = all forward
 *   feat    float (n,128)  features carried from each particle's first window
 *   active  int32 (n_act)  the particles of this hop: strictly ascending indices into [0, n)
 * The library does not verify `active` (that would take a pass over device memory): ascending order is the caller's to keep.
 * A member outside [0, n) is never dereferenced and is IGNORED -- the gather stages zeros for it, the step writes no row, no
 * cur / feat / steps element and never lists it in next_active -- so a corrupt list cannot write out of bounds; the tracker
 * still runs a window for it, and its results are dropped.  Frame arithmetic (cur + dir * s, f + base) is plain int: keep
 * |cur| + |base| + 8 below 2^31.
 * L >= 8 keeps the 8 rows of a window apart.  A linear buffer over a video of T frames with windows that may run past either
 * end is L = T + 14, base = 7; a ring over a streamed video is base = 0 with the caller reusing rows.
 *
 * pips_chain_hop = pips_chain_gather, pips_track_ring on (B = 1, N = n_act) windows, pips_chain_step, on `stream`:
 *   sample_feat != 0  the windows sample their features at the start positions (feat_init = NULL) and feat[q] receives them
 *                     (a particle's first window); 0: the windows run on feat[q], which stays as it is
 *   next_active       int32, room for n_act: the members of active with 0 <= cur < T after the step, IN THEIR ORDER
 *                     (a block scan, not atomics); may not alias active; elements past *next_count are not written
 *   next_count        device int32: their number.  The library does not synchronise: the caller copies it back
 *   steps             int32 (n_act) or NULL: the step si in 2..7 of each active particle (7 for NaN logits, as the reference's
 *                     comparison admits no frame)
 * n_act == 0: PIPS_OK, *next_count = 0, nothing else.  PIPS_E_ARG: n_act < 0 or > n, L < 8, R < 1, T < 1, a map below 16 x 16
 * (pips_chain_hop: the map size rule at pips_forward), a NULL active / trajs / cur / feat / next_active / next_count; PIPS_E_WORKSPACE: workspace_bytes < pips_chain_workspace_bytes(n_act, iters)
 * (= pips_track_workspace_bytes_s(1, n_act, 8) + the staging arrays and the windows).  A rejected call writes nothing.
 * pips_chain_threshold(k), k in 0..63: the k-th threshold (host function; the subtraction in double, rounded to fp32).
 * The two stages on their own (parity tests):
 *   pips_chain_gather  xy (n_act,2) = trajs[row(cur[q]), q], ws = cur[q], wd = dir ? dir[q] : 1, fi (n_act,128) = feat[q]
 *                      (fi is not written with sample_feat): the xys / win_start / win_dir / feat_init of pips_track_ring
 *   pips_chain_step    win_trajs (8,n_act,2), win_vis (8,n_act), win_ffeat0 (n_act,128; read with sample_feat): the write-back,
 *                      scan, cur / feat update and compaction; every other element of trajs / vis stays bit-identical */
float  pips_chain_threshold(int k);
size_t pips_chain_workspace_bytes(int n_act, int iters);
int    pips_chain_gather(const float* trajs, int L, int base, int n, const int* cur, const int* dir, const float* feat,
                         const int* active, int n_act, int sample_feat, float* xy, int* ws, int* wd, float* fi, void* stream);
int    pips_chain_step(const float* win_trajs, const float* win_vis, const float* win_ffeat0, int T, int n, const int* active,
                       int n_act, int sample_feat, float* trajs, float* vis, int L, int base, int* cur, const int* dir,
                       float* feat, int* next_active, int* next_count, int* steps, void* stream);
int    pips_chain_hop(const void* arena, const float* pyramid, int T, int R, int H8, int W8,
                      const float* times, int stride, int iters, int flags,
                      int n, const int* active, int n_act, int sample_feat,
                      float* trajs, float* vis, int L, int base,
                      int* cur, const int* dir, float* feat,
                      int* next_active, int* next_count, int* steps,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same for a state that holds the particles of V videos (pips_track_clips: one flat linear cache, T = all its frames, R = T):
 *   clip        int32 (n)  the video of each particle, or NULL (= the forms above; the tables and V are then not read)
 *   clip_first / clip_frames / V   the clip table of pips_track_clips
 * cur counts frames of the particle's own video and a particle stays live while 0 <= cur < clip_frames[clip[q]] (clip[q] clamped
 * to [0, V-1]) instead of < T.  trajs / vis stay (L,n,2) / (L,n) with one base: L is sized for the LONGEST video (L = max
 * clip_frames + 14, base = 7), and a particle of a shorter video finishes while the others go on.  pips_chain_gather_clips also
 * stages wc (n_act) = clip[q] (0 for a member outside [0, n)), the win_clip of pips_track_clips.  Compaction order, NaN handling
 * and the thresholds are those of the forms above.  With clip, PIPS_E_ARG ahead of any launch also for: V < 1, a NULL clip_first
 * (hop) / clip_frames (hop, step) / wc (gather), R != T (hop). */
int    pips_chain_gather_clips(const float* trajs, int L, int base, int n, const int* cur, const int* dir, const int* clip,
                               const float* feat, const int* active, int n_act, int sample_feat, float* xy, int* ws, int* wd,
                               int* wc, float* fi, void* stream);
int    pips_chain_step_clips(const float* win_trajs, const float* win_vis, const float* win_ffeat0, int T, int n,
                             const int* active, int n_act, int sample_feat, float* trajs, float* vis, int L, int base, int* cur,
                             const int* dir, const int* clip, const int* clip_frames, int V, float* feat, int* next_active,
                             int* next_count, int* steps, void* stream);
int    pips_chain_hop_clips(const void* arena, const float* pyramid, int T, int R, int H8, int W8,
                            const float* times, int stride, int iters, int flags,
                            int n, const int* active, int n_act, int sample_feat,
                            float* trajs, float* vis, int L, int base,
                            int* cur, const int* dir,
                            const int* clip, const int* clip_first, const int* clip_frames, int V,
                            float* feat, int* next_active, int* next_count, int* steps,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- streamed chaining: one call per round ------------------------------------------------
 * Replaces: the per-round bookkeeping of a tracker that follows query points through a video that arrives in chunks -- the
 * forward chains of chain_demo.py:40-83 from each query's own frame, run while frames are still being appended to a ring of R
 * frame slots (pips_pyramid_append) and handed out as soon as no pending window can change them.  Which queries have their 8
 * window frames, which of them start with this round (their start row and first-window features), the hop itself
 * (pips_chain_hop, base = 0), which queries are finished and which frames are final are all decided here; the host reads four
 * ints per round.
 *
 * The caller owns the state, all of it on the device, for n queries:
 *   tq      int32 (n)      query frame
 *   xy      float (n,2)    query position, pixels
 *   cur     int32 (n)      window start; the caller sets cur = tq, the hops advance it
 *   status  int32 (n)      0 = waiting, 1 = joined, 2 = done; the caller sets 0
 *   feat    float (n,128)  features of each query's first window (written when it joins)
 *   trajs   float (L,n,2)  logical frame f lives in row f mod L (base = 0); L >= 16
 *   vis     float (L,n)    visibility logits, same rows
 *   active / new_list  int32, room for n each;  counts  int32 (4) = {n_act, n_new, low, 0}
 * n grows by the caller re-allocating the arrays and copying (new queries: cur = tq, status 0, rows as the caller fills unused
 * rows); the library only sees a larger n.
 *
 * pips_stream_select, the first call after an append (T = logical frames appended so far), one pass over the n queries:
 *   final != 0: a joined query with cur >= T becomes done (status 2)
 *   a query is READY when it is not done and (final ? cur < T : cur + 8 <= T)
 *   active   <- the ready queries, ascending;  new_list <- the ready queries with status 0, ascending (a block scan, not
 *               atomics); elements past the counts are not written
 *   for each member of new_list: trajs[tq mod L, q] = xy[q], status = 1
 *   counts[0] = n_act, counts[1] = n_new, counts[2] = low = min cur over the queries that are not done (INT_MAX: none), counts[3] = 0
 * pips_stream_round(n_act, n_new as read from counts), on `stream`:
 *   join     feat[q] for q in new_list[0..n_new) = the point sample of pips_track_ring(feat_init = NULL, win_start = tq[q],
 *            iters = 0) at xy[q]
 *   hop      pips_chain_hop over active[0..n_act) with sample_feat = 0, base = 0, dir = NULL; steps int32 (n_act) or NULL
 *            receives the step of each active query
 *   select   pips_stream_select(T, final) again: active / new_list / counts hold the NEXT round
 * The loop of one append (or of the end of the video, final = 1): select, copy counts back, then round and copy counts back
 * while counts[0] > 0 -- one host read per round.  With counts[0] == 0, frames [emitted, min(low, T)) are final:
 * pips_stream_emit(f0, f1), 0 <= f1 - f0 <= L, copies rows f mod L of trajs / vis to the dense out_trajs (f1-f0, n, 2) /
 * out_vis (f1-f0, n) and stores the fp32 quiet NaN 0x7fc00000 into those rows; every other row stays bit-identical.  Rows whose
 * length is a multiple of 16 bytes (in 16-byte aligned buffers) move as 16-byte pieces, other rows word by word.
 *
 * The caller keeps true:
 *   - no frame slot is overwritten while a pending window can read it: append at most up to T <= low + R (low of the last counts;
 *     with R >= 9 this always leaves room for one new frame);
 *   - the final rounds are not started with a waiting query whose tq >= T (it could never join: the loop would end with it
 *     pending and its frames never final);
 *   - tq >= 0 and tq >= the first frame not yet emitted when a query is added; |cur| + 8 below 2^31.
 * A member of active / new_list outside [0, n) is never dereferenced (pips_chain_hop's rule).
 * n_act == 0 (round) or f0 == f1 (emit): PIPS_OK and nothing is done.  PIPS_E_ARG ahead of any launch: n < 1; n_act or n_new
 * outside [0, n]; n_new > n_act; L < 16; R < 9; T < 1; a map below 16 x 16 (round: the map size rule at pips_forward); f1 < f0 or
 * f1 - f0 > L; f1 - f0 > PIPS_STREAM_EMIT_FRAMES_MAX (emit puts a frame on each of the grid's rows of blocks: a longer ring is
 * emitted in several calls); a NULL array (steps may be NULL).
 * PIPS_E_WORKSPACE: workspace_bytes < pips_stream_workspace_bytes(n, iters) (= pips_chain_workspace_bytes(n, iters) + the staging
 * of the join + the hop's unused compacted list).  A rejected call writes nothing.  No allocation, no synchronisation. */
size_t pips_stream_workspace_bytes(int n, int iters);
int    pips_stream_select(int T, int final, int n, const int* tq, const float* xy, int* cur, int* status, float* trajs, int L,
                          int* active, int* new_list, int* counts, void* stream);
int    pips_stream_round(const void* arena, const float* pyramid, int T, int R, int H8, int W8,
                         const float* times, int stride, int iters, int flags, int final,
                         int n, int n_act, int n_new,
                         const int* tq, const float* xy, int* cur, int* status, float* feat,
                         float* trajs, float* vis, int L,
                         int* active, int* new_list, int* counts, int* steps,
                         void* workspace, size_t workspace_bytes, void* stream);
int    pips_stream_emit(float* trajs, float* vis, int L, int n, int f0, int f1, float* out_trajs, float* out_vis, void* stream);
/* Several streams in one state: V videos of one frame size, each with its own length and its own end, on one flat cache of V
 * rings of R slots (pips_track_rings).  The state of pips_stream_round, plus
 *   clip        int32 (n)  the stream of each query (clamped to [0, V-1] where it is read)
 *   clip_first  int32 (V)  first flat slot of each stream's ring
 *   clip_frames int32 (V)  logical frames appended to each stream so far (the T of that stream's queries)
 *   clip_final  int32 (V)  != 0: the stream has ended (the `final` of that stream's queries)
 *   counts      int32 (4 + V) = {n_act, n_new, low over all streams, 0, low_0 .. low_{V-1}}; low_v = min cur over the queries of
 *               stream v that are not done (INT_MAX: none)
 * cur, tq and the rows of trajs / vis (frame f in row f mod L) count frames of the query's OWN stream.  A query of stream v is
 * done / ready by pips_stream_select's rule with T = clip_frames[v] and final = clip_final[v]; the lists keep their ascending order
 * (the same block scan).  The round stages clip[q] next to tq[q] for the join's point sample and hops with the clip table
 * (pips_chain_hop over pips_track_rings).  The host loop of one wave of appends: pips_pyramid_append_at per stream (and the new
 * clip_frames), pips_stream_select_clips, the counts copied back, then pips_stream_round_clips and the counts copied back while
 * counts[0] > 0; frames [emitted_v, min(low_v, clip_frames[v])) of stream v are then final: pips_stream_emit_cols on its columns.
 * Each stream keeps pips_stream_round's rules on its own (append up to clip_frames[v] <= low_v + R; no final rounds with a waiting
 * query whose tq >= clip_frames[v]).  V <= PIPS_STREAM_V_MAX.
 * PIPS_E_ARG ahead of any launch: what pips_stream_select / pips_stream_round answer it for, V < 1 or > PIPS_STREAM_V_MAX, a NULL
 * clip / table, F < V*R.  PIPS_E_WORKSPACE: workspace_bytes < pips_stream_workspace_bytes_clips(n, iters, V) (0 for a V outside
 * the range).  A rejected call writes nothing.
 * pips_stream_emit_cols: pips_stream_emit for the columns cols[0..m) only (device int32, ascending, not verified) -- streams become
 * final at different frames.  Rows f mod L, f in [f0, f1), of those columns go to the dense out_trajs (f1-f0, m, 2) / out_vis
 * (f1-f0, m) as bit patterns, and 0x7fc00000 is stored back into exactly those elements; every other element stays bit-identical.
 * A member of cols outside [0, n) is skipped: nothing is read or reset, and its output elements receive the same NaN.  f0 == f1
 * or m == 0: PIPS_OK and nothing is done.  PIPS_E_ARG: n < 1, L < 16, m < 0, f1 < f0, f1 - f0 > L or
 * > PIPS_STREAM_EMIT_FRAMES_MAX, a NULL array. */
#define PIPS_STREAM_V_MAX 64
#define PIPS_STREAM_EMIT_FRAMES_MAX 65535
size_t pips_stream_workspace_bytes_clips(int n, int iters, int V);
int    pips_stream_select_clips(int n, const int* tq, const float* xy, int* cur, int* status, const int* clip,
                                const int* clip_frames, const int* clip_final, int V, float* trajs, int L,
                                int* active, int* new_list, int* counts, void* stream);
int    pips_stream_round_clips(const void* arena, const float* pyramid, int F, int R, int H8, int W8,
                               const float* times, int stride, int iters, int flags,
                               int n, int n_act, int n_new,
                               const int* tq, const float* xy, int* cur, int* status, const int* clip, float* feat,
                               float* trajs, float* vis, int L,
                               const int* clip_first, const int* clip_frames, const int* clip_final, int V,
                               int* active, int* new_list, int* counts, int* steps,
                               void* workspace, size_t workspace_bytes, void* stream);
int    pips_stream_emit_cols(float* trajs, float* vis, int L, int n, int f0, int f1, const int* cols, int m,
                             float* out_trajs, float* out_vis, void* stream);
/* Queries leave a running stream: pips_stream_keep copies the columns keep[0..m) (device int32, strictly ascending, not verified;
 * 0 <= m <= n) of the state of pips_stream_round / pips_stream_round_clips for n queries into caller-owned arrays sized for m
 * queries -- tq_out / cur_out / status_out (m), xy_out (m,2), feat_out (m,128), trajs_out (L,m,2), vis_out (L,m), and clip_out (m)
 * with clip -- none of which may alias an input.  Column j of every output is column keep[j] of the input: the integer arrays, xy
 * and feat verbatim, the rows of trajs / vis as bit patterns (NaN payloads survive, as in pips_stream_emit); the inputs stay
 * bit-identical, and the caller releases them and goes on with the narrower state (active / new_list / steps need room for m, the
 * workspace is sized for m).  counts receives {0, 0, low, 0[, low_0 .. low_{V-1}]}: low = min cur over the kept queries whose
 * status is not 2 (INT_MAX: none), low_v the same over those of stream v (clip clamped to [0, V-1]) -- what pips_stream_select*
 * would report for the kept set, so the host sizes its next append without a select (a second select would mark waiting queries
 * joined without their join having run: this entry point never selects).  clip == NULL: the one-stream state -- V and clip_out are
 * not read, counts has 4 ints; with clip, 1 <= V <= PIPS_STREAM_V_MAX and counts has 4 + V.
 * A member of keep outside [0, n) is never dereferenced: its output column becomes a finished, empty query -- status 2, tq = cur = 0,
 * clip = 0, xy and feat zero, rows 0x7fc00000 (pips_stream_emit_cols' rule for a bad column) -- and enters no low.
 * m == 0: PIPS_OK, only counts is written (keep and the *_out arrays are not looked at).  PIPS_E_ARG ahead of any launch: n < 1,
 * m < 0, m > n, L < 16, a NULL array (clip and clip_out are NULL together or not at all), V out of range with clip.  A rejected
 * call writes nothing.  Two launches; no allocation, no synchronisation, no workspace. */
int    pips_stream_keep(int n, const int* keep, int m,
                        const int* tq, const float* xy, const int* cur, const int* status, const int* clip, const float* feat,
                        const float* trajs, const float* vis, int L,
                        int* tq_out, float* xy_out, int* cur_out, int* status_out, int* clip_out, float* feat_out,
                        float* trajs_out, float* vis_out,
                        int V, int* counts, void* stream);
/* Keeping the frame covered: pips_cover_step judges the n queries of a stream on the frames [f1 - m, f1) that were just moved out
 * of its row ring (pips_stream_emit's dense trajs (m,n,2) / vis (m,n)), and lists the cells of a grid over the H x W frame that
 * need a new query.  The grid has gh = ceil(H / cell) rows and gw = ceil(W / cell) columns, row-major; with f = f1 - 1:
 *  - a query with tq > f is PENDING: kept, its run 0, standing on its query position xy (every query of a step with m = 0 is);
 *  - a started query updates its run over the returned frames g >= tq in order, run = (vis[g] < vis_logit) ? run + 1 : 0,
 *    starting from lost[c] (a NaN compares false and resets the run; vis_logit is logit(threshold), computed by the host), and
 *    stands on (x, y) = trajs[f].  It is retired as OUTSIDE unless x >= 0 && x <= W-1 && y >= 0 && y <= H-1 (NaN and +-inf
 *    retire), otherwise as LOST if run >= lost_after (INT_MAX: never), otherwise kept;
 *  - a kept query whose position passes the same test occupies the cell (min(int(floor(y / cell)), gh-1), min(int(floor(x /
 *    cell)), gw-1)), `/` being the correctly rounded fp32 quotient by float(cell); a pending query outside the frame occupies none.
 * keep[0..n_keep) receives the kept columns, strictly ascending, and lost_out[0..n_keep) their runs in that order -- keep is the
 * list pips_stream_keep takes, lost_out the `lost` of the narrower state.  seeds receives one (t, x, y) = (f1, min((j + 0.5) *
 * cell, W-1), min((i + 0.5) * cell, H-1)) per cell (i, j) that nobody occupies, in row-major order, cut after max(0,
 * max_queries - n_keep) entries: the (1,n_seed,3) queries to add.  counts = {n_keep, n_seed, n_outside, n_lost}, outside taking
 * precedence over lost.  keep and lost_out need room for n ints, seeds for min(gh*gw, max_queries) triples; the elements behind
 * the counts are not written.  Every input stays bit-identical, `lost` included.  The first step of a stream runs before anything
 * is encoded, with m = 0 and f1 = 0: the seeds land on frame 0.  n = 0 is a valid call (tq, xy, lost, keep and lost_out are then
 * not looked at; trajs and vis are not looked at when m = 0 or n = 0).
 * PIPS_E_ARG ahead of any launch: n < 0, m < 0, cell < 8, H or W < 1, lost_after < 1, max_queries < 0, m == 0 with f1 != 0,
 * f1 < m, more than PIPS_COVER_CELLS_MAX cells, a NULL array that would be read or written.  PIPS_E_WORKSPACE: workspace_bytes <
 * pips_cover_workspace_bytes(n, gh, gw) (0 for n < 0, gh or gw < 1, too many cells).  A rejected call writes nothing.  One memset
 * node and two launches; the lists are scanned by one block (their order is the contract); no allocation, no synchronisation. */
#define PIPS_COVER_CELLS_MAX (1 << 24)
size_t pips_cover_workspace_bytes(int n, int gh, int gw);
int    pips_cover_step(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy,
                       const int* lost, int H, int W, int cell, float vis_logit, int lost_after, int max_queries,
                       int* keep, int* lost_out, float* seeds, int* counts,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The thin cover step: pips_cover_step with a cap of per_cell tracks in a cell.  Tracks that lose their surface slide onto a
 * neighbour and ride along with it; pips_cover_step re-seeds the cell they left and never removes the duplicates where they
 * arrive.  pips_cover_step_thin extends that rule and replaces none of it.  In its notation (rows of frames [f1 - m, f1), f =
 * f1 - 1, the gh x gw grid, the fp32 quotient, the inside test 0 <= x <= W-1 && 0 <= y <= H-1 that NaN and +-inf fail):
 *  1. pending, the flags OUTSIDE and LOST and the run `lost` are exactly pips_cover_step's;
 *  2. a query COUNTS on a returned frame g when it is not pending, tq <= g, it is not flagged outside or lost in this step and
 *     its position trajs[g] passes the inside test; its cell on g is (min(int(floor(y / cell)), gh-1), min(int(floor(x / cell)), gw-1));
 *  3. a counting query j is SURPLUS on g when at least per_cell counting queries i < j stand in j's cell on g -- columns are in
 *     order of creation, so the lower column is the older identity; a query that does not count on g is not surplus on g;
 *  4. a second run is carried from push to push beside `lost`: over the returned frames g >= tq in order, run = surplus ? run + 1
 *     : 0, starting from crowd[c]; it is 0 for a pending query;
 *  5. a started query that is neither outside nor lost is retired as CROWDED when that run >= crowd_after;
 *  6. occupancy, the seeds, their row-major order and the cap are pips_cover_step's with "kept" also excluding the crowded: a
 *     crowded query that stood alone in its cell on f frees that cell for a seed of this very step, and the cap is max(0,
 *     max_queries - n_keep) with the new n_keep.
 * The rule is NOT greedy: an elder counts on a row even when it is itself retired as crowded in this step (only outside and lost
 * take it out of the count), so the rank by age is well defined without a sequential pass over the queries.  The rule is per cell,
 * not per distance: seeds go only into empty cells, so a seed is never surplus where it is born.  Its known limit: two tracks 1 px
 * apart on either side of a cell border are not merged.  With per_cell = INT_MAX nobody is surplus and keep, lost_out, seeds and
 * the first four counts are pips_cover_step's bit for bit.
 * crowd (n) is the second run of each query (0 for a new one), crowd_out[0..n_keep) that of the kept, aligned with keep and
 * lost_out.  gone[0..n - n_keep) receives the retired columns, ascending, and reason[.] why: 1 outside, 2 lost, 3 crowded (the
 * precedence in that order).  counts = {n_keep, n_seed, n_outside, n_lost, n_crowded}.  keep, lost_out, crowd_out, gone and reason
 * need room for n ints each; the elements behind the counts are not written; every input stays bit-identical.
 * PIPS_E_ARG ahead of any launch: pips_cover_step's cases, per_cell < 1, crowd_after < 1, a NULL crowd, crowd_out, gone or reason
 * (n > 0).  PIPS_E_WORKSPACE: workspace_bytes < pips_cover_thin_workspace_bytes(n, m, gh, gw) (0 for n < 0, m < 0, gh or gw < 1,
 * too many cells) -- pips_cover_workspace_bytes plus a run per query and a surplus bit per (row, query).  A rejected call writes
 * nothing.  One memset node and at most four launches (m = 0 skips the ranking, n = 0 everything but the lists); a block of 256 queries
 * ranks itself against the older ones of one row through LDS; the lists are scanned by one block; no atomics, no allocation, no
 * synchronisation. */
size_t pips_cover_thin_workspace_bytes(int n, int m, int gh, int gw);
int    pips_cover_step_thin(int n, int m, int f1, const float* trajs, const float* vis, const int* tq, const float* xy,
                            const int* lost, const int* crowd, int H, int W, int cell, float vis_logit, int lost_after,
                            int max_queries, int per_cell, int crowd_after,
                            int* keep, int* lost_out, int* crowd_out, float* seeds, int* gone, int* reason, int* counts,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Seeding on corners: pips_corner_table looks at the pixels of F frames (F,3,h,w), planar, uint8 (src_is_u8 != 0) or float32 with
 * values 0..255 (finite), and writes table (F,gh,gw,3) = (x, y, S) -- the most trackable pixel of each cell of pips_cover_step's
 * grid (gh = (h-1)/cell + 1 rows, gw likewise) and its score.  Everything up to the argmax is integer arithmetic:
 *  - a float channel is quantised as u = floor(min(max(v, 0), 255) + 0.5); luma Y = (77 R + 150 G + 29 B + 128) >> 8;
 *  - gx = Y[y][x+1] - Y[y][x-1], gy = Y[y+1][x] - Y[y-1][x]; over the 7x7 window centred on the pixel a = sum gx^2, b = sum gx gy,
 *    c = sum gy^2 (int32); S = a + c - ceil(sqrt((a-c)^2 + 4 b^2)), the root exact (int64): twice the smaller eigenvalue of the
 *    structure tensor rounded down, 0 <= S <= 6 372 450, exact as a float;
 *  - the candidates are the pixels with 4 <= x <= w-5 and 4 <= y <= h-5 (every read lies inside the frame); cell (i, j) covers
 *    rows [i cell, (i+1) cell) and columns [j cell, (j+1) cell) clipped to the frame, and its entry is the candidate with the
 *    largest S -- among equals the lowest y, then the lowest x;
 *  - a cell without a candidate holds pips_cover_step's centre (min((j + 0.5) cell, w-1), min((i + 0.5) cell, h-1)) and S = -1.
 * With an unweighted window the best pixel of a sharp corner lies about 2 px inside it, not on it.
 * pips_cover_place moves the k seeds (t, x, y) that pips_cover_step wrote for frame t onto table_of_frame (gh,gw,3), the part of
 * the table that belongs to frame t: a seed belongs to cell (min(int(floor(y / cell)), gh-1), min(int(floor(x / cell)), gw-1)),
 * the fp32 quotient of pips_cover_step (it finds the cell of a clamped centre too), and takes that entry's (x, y) if its S >
 * min_corner; otherwise it stays where it is.  t is not looked at; the number and the order of the seeds do not change.
 * PIPS_E_ARG ahead of any launch: F < 0, k < 0, h or w < 1, cell < 8, min_corner < 0, a NULL pointer, a frame of more than
 * INT_MAX pixels, more than PIPS_CORNER_BLOCKS_MAX cells in all frames of a call (a launch takes at most 2^32 threads, a cell
 * is a block of 256: split the chunk).  A rejected call writes nothing; F = 0 and k = 0 launch nothing and return
 * PIPS_OK.  One launch each -- a 256-thread block per (frame, cell) / a thread per seed; no atomics, no workspace, no
 * allocation, no synchronisation. */
#define PIPS_CORNER_BLOCKS_MAX ((1 << 24) - 1)
int    pips_corner_table(const void* frames, int src_is_u8, int F, int h, int w, int cell, float* table, void* stream);
int    pips_cover_place(float* seeds, int k, const float* table_of_frame, int h, int w, int cell, int min_corner, void* stream);
/* Scene cuts: pips_cut_table looks at the pixels of F frames (F,3,h,w) -- pips_corner_table's input: planar, uint8 (src_is_u8 != 0)
 * or float32 with values 0..255 -- and writes hist (F,16,32) int32, the regional luma histogram of each frame, and dist (F) int32,
 * its distance to the frame before.  Integers only:
 *  - pips_corner_table's luma: a float channel is quantised as u = floor(min(max(v, 0), 255) + 0.5), Y = (77 R + 150 G + 29 B +
 *    128) >> 8;
 *  - pixel (y, x) counts in region r = 4 ((4 y) / h) + (4 x) / w (integer division: a 4 x 4 grid over the frame, with empty
 *    regions when h or w < 4) and bin b = Y >> 3: hist[f][r][b] is the number of such pixels, and a frame's counts sum to h w;
 *  - dist[f] = sum over (r, b) of |hist[f][r][b] - hist[f-1][r][b]| for f >= 1; dist[0] is taken against prev_hist (16,32), the
 *    last histogram of the call before, or is 0 when prev_hist is NULL.  0 <= dist <= 2 h w (stored as its low 32 bits: 2^31 is
 *    reached only by a frame of exactly 2^30 pixels that shares no bin with its neighbour in any region).
 * A caller puts a cut before frame f iff dist[f] > limit with limit = floor(cut_thr * 2 h w) computed once on the host in double
 * (drivers.Cover(cut_thr=), drivers.find_cuts); the library knows no threshold.
 * Two launches: 4 * S blocks of 256 threads per frame count S strips of pixel rows of each of the 4 region rows (S = min(16,
 * max(1, (ceil(h / 4) + 7) / 8))) in LDS and store their partial histograms -- 128 int32 each -- to the workspace with plain
 * stores; then a block per frame sums the partials of frames f and f-1 in a fixed order, writes hist[f] and reduces dist[f].
 * Rows are read with 16-byte loads where a frame's three planes share their alignment (plane bytes a multiple of 16), from the
 * first 16-byte address of each row on; every other pixel, row width and base address takes element loads.  No global atomics, no
 * allocation, no synchronisation; nothing but hist, dist and the first pips_cut_workspace_bytes(F, h, w) bytes of the workspace
 * (= F * 4 * S * 512; 0 for arguments that pips_cut_table rejects) is written, and prev_hist may not overlap them.
 * PIPS_E_ARG ahead of any launch: F < 0 or > PIPS_CUT_FRAMES_MAX, h or w < 1, h w > 2^30, and with F > 0 a NULL frames, hist,
 * dist or workspace.  PIPS_E_WORKSPACE: workspace_bytes < pips_cut_workspace_bytes(F, h, w).  A rejected call writes nothing; F =
 * 0 launches nothing and returns PIPS_OK. */
#define PIPS_CUT_FRAMES_MAX ((1 << 25) - 1)
size_t pips_cut_workspace_bytes(int F, int h, int w);
int    pips_cut_table(const void* frames, int src_is_u8, int F, int h, int w, const int32_t* prev_hist, int32_t* hist, int32_t* dist,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- stages (same kernels, exposed for parity tests and for callers that cache maps) --*/

/* BasicEncoder.forward (nets/pips.py:247-281) incl. the 2*(x/255)-1 of :436 and
 * CorrBlock.__init__ (:346-352).  Writes the 4-level channel-last pyramid:
 * level l at pyramid + pips_pyramid_offset(l), shape [F][H_l][W_l][128]. */
size_t pips_encoder_workspace_bytes(int F, int H, int W, int stride);
size_t pips_pyramid_floats(int F, int H, int W, int stride);
size_t pips_pyramid_offset(int F, int H, int W, int stride, int level);   /* in floats */
/* pips_pyramid_floats = the four fp32 levels + their bf16 mirror (same element offsets, half the bytes) behind them */
size_t pips_pyramid_mirror_offset(int F, int H, int W, int stride);       /* in floats: where the mirror starts = size of the fp32 levels */
int    pips_pyramid_mirror(float* pyramid, int F, int H, int W, int stride, void* stream);   /* (re)write the mirror from the fp32 levels */
/* Streamed video: copy the levels of k frames just encoded (src: a pips_encoder_fwd* pyramid of F = k frames) into slots
 * (T0 + i) mod R, i < k, of a ring pyramid of R frame slots (pips_pyramid_floats(R, ...)), wrapping past slot R-1, and write
 * the bf16 mirror of those slots from the fp32 levels in the same pass (pips_pyramid_mirror's rounding).  One launch.
 * Needs R >= 1, T0 >= 0 and 1 <= k <= R. */
int    pips_pyramid_append(const float* src, int k, float* ring, int R, int T0, int H, int W, int stride, void* stream);
/* The same between two positions: frames [src_first, src_first + k) of an encoder pyramid of F_src frames go into slots
 * ring_first + (T0 + i) mod R, i < k, of a pyramid laid out for F slots (one ring of a cache of several, pips_track_rings), the
 * bf16 mirror of those slots in the same pass.  One launch.  Checks as pips_pyramid_append, plus 0 <= src_first, src_first + k <=
 * F_src, 0 <= ring_first and ring_first + R <= F: both ranges lie inside their buffers. */
int    pips_pyramid_append_at(const float* src, int F_src, int src_first, int k, float* dst, int F, int ring_first, int R, int T0,
                              int H, int W, int stride, void* stream);
int    pips_encoder_fwd(const void* arena, const float* rgbs, int F, int H, int W, int stride,
                        float* pyramid, void* workspace, size_t workspace_bytes, void* stream);

int    pips_encoder_fwd_bf16(const void* arena, const float* rgbs, int F, int H, int W, int stride,
                             float* pyramid, void* workspace, size_t workspace_bytes, void* stream);
/* general form: flags = PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_RGB_U8 */
int    pips_encoder_fwd_ex(const void* arena, const void* rgbs, int F, int H, int W, int stride, int flags,
                           float* pyramid, void* workspace, size_t workspace_bytes, void* stream);

/* The callers' frame pre-processing (demo.py:22-28, chain_demo.py:26-28, test_on_davis.py:93-95):
 * F.interpolate(rgbs, (H,W), mode='bilinear') (align_corners=False) of decoded frames, on the device.
 * src: planes = F*3 images of h x w, uint8 (src_is_u8 != 0) or float; dst: float (planes,H,W), values 0..255,
 * i.e. exactly what pips_forward / pips_encoder_fwd take as rgbs. */
int    pips_resize_frames(const void* src, int src_is_u8, int planes, int h, int w,
                          float* dst, int H, int W, void* stream);

/* Decoder frames in: pips_frames_import takes F frames of h x w in the layout a decoder, a camera or an image library hands over
 * and writes dst (F,3,H,W), planar and contiguous, uint8 (dst_is_u8 != 0) or float32 with values 0..255 -- the frames that
 * pips_encoder_fwd_ex (PIPS_FLAG_RGB_U8 for uint8), pips_forward, pips_corner_table and pips_cut_table read.  Integers only up to
 * the resize:
 *  - addressing: frame f, row y of source plane k starts at p_k + f step_k + y pitch_k (bytes).  Any base address, any pitch >= the
 *    bytes of a row and any step >= pitch_k x rows_k: no alignment is asked for.  Planes a format does not have are not read and
 *    may be NULL with zero pitch and step;
 *  - PIPS_FMT_RGB24, BGR24, RGBA32, BGRA32 (packed, bpp = 3 or 4): pixel (y, x) is the bpp bytes at x bpp of row y of plane 0; R, G,
 *    B are bytes 0, 1, 2 for RGB / RGBA and bytes 2, 1, 0 for BGR / BGRA; the alpha byte is never read.  matrix and range are not
 *    looked at;
 *  - PIPS_FMT_NV12: Y = plane0[y][x]; Cb = plane1[y >> 1][2 (x >> 1)] and Cr the byte behind it: plane 1 has ceil(h / 2) rows of
 *    2 ceil(w / 2) bytes.  PIPS_FMT_I420: Y likewise, Cb = plane1[y >> 1][x >> 1], Cr = plane2[y >> 1][x >> 1]: planes of ceil(h / 2)
 *    rows of ceil(w / 2) bytes.  Odd h and w are legal;
 *  - YCbCr -> RGB: c = Y - y0 (y0 = 16 for PIPS_RANGE_LIMITED, 0 for PIPS_RANGE_FULL), d = Cb - 128, e = Cr - 128,
 *      R = clamp((ky c + rv e + 32768) >> 16), G = clamp((ky c + gu d + gv e + 32768) >> 16), B = clamp((ky c + bu d + 32768) >> 16)
 *    with >> the arithmetic shift (floor), clamp to [0, 255], and the constants floor(65536 k + 0.5) of the standard coefficients
 *    (luma scaled by 255/219 and chroma by 255/224 in limited range):
 *                                 ky      rv      gu      gv      bu
 *      PIPS_MATRIX_BT601 limited  76309  104597  -25675  -53279  132201
 *      PIPS_MATRIX_BT601 full     65536   91881  -22553  -46802  116130
 *      PIPS_MATRIX_BT709 limited  76309  117489  -13975  -34925  138438
 *      PIPS_MATRIX_BT709 full     65536  103206  -12276  -30679  121609
 *    Over all 2^24 triples every accumulator stays inside int32 (-1.9e7 .. 3.6e7), and the result is at most one level away from
 *    clamp(floor(exact + 0.5)) of the real-valued formula;
 *  - H == h and W == w: dst holds the 8-bit value, as a uint8 or as the same value in a float.  Otherwise the float dst is
 *    pips_resize_frames' arithmetic on the converted 8-bit planes -- sh = (float)h / (float)H, fy = max(sh (y + 0.5) - 0.5, 0)
 *    with the product and the difference one fused multiply-add, y0 = min((int)fy, h - 1), y1 = y0 + (y0 < h - 1), the same for x,
 *    weights ly1 = fy - y0 and ly0 = 1 - ly1, and v = ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11): four single-rounded fp32
 *    products and three sums in that order, none fused -- bit for bit what
 *    importing at (h, w) as uint8 and pips_resize_frames on that gives; the uint8 dst is floor(v + 0.5) of that float (v lies in
 *    [0, 255]), the quantisation pips_corner_table and pips_cut_table apply to a float frame: they give the same integers on the
 *    uint8 and on the float output of one import.
 * pips_frames_import_ex is the same entry with a filter argument and two more formats (pips_frames_import is
 * pips_frames_import_ex with PIPS_FILTER_BILINEAR and keeps rejecting formats above PIPS_FMT_I420):
 *  - PIPS_FMT_P010 (semi-planar as NV12) and PIPS_FMT_I010 (planar as I420, yuv420p10le): samples are 16-bit little-endian words,
 *    the 10-bit value is word >> 6 for P010 and word & 1023 for I010 (the other six bits are not looked at).  Geometry and chroma
 *    replication are NV12's and I420's; pitches and steps stay in bytes: a row of Y is 2 w bytes, a row of P010's chroma
 *    2 x 2 ceil(w / 2) and of I010's 2 ceil(w / 2).  Every plane pointer, pitch and step of these two formats must be even;
 *  - 10-bit YCbCr -> the same 8-bit RGB: c = Y - y0 (y0 = 64 limited, 0 full), d = Cb - 512, e = Cr - 512,
 *      R = clamp((ky c + rv e + 2^17) >> 18), G = clamp((ky c + gu d + gv e + 2^17) >> 18), B = clamp((ky c + bu d + 2^17) >> 18)
 *    with the constants floor(2^18 k + 0.5) of the standard coefficients, luma scaled by 255/876 and chroma by 255/896 in limited
 *    range and both by 255/1023 in full range:
 *                                         ky      rv      gu      gv      bu
 *      10-bit PIPS_MATRIX_BT601 limited   76309  104597  -25675  -53279  132201
 *      10-bit PIPS_MATRIX_BT601 full      65344   91612  -22487  -46664  115789
 *      10-bit PIPS_MATRIX_BT709 limited   76309  117489  -13975  -34925  138438
 *      10-bit PIPS_MATRIX_BT709 full      65344  102903  -12240  -30589  121252
 *    The limited rows are the 8-bit constants: a limited-range surface whose samples are 4 x the bytes of an 8-bit one imports to
 *    the same frames (in full range 4 x 255 is not 1023: the two differ by design).  Every accumulator stays inside int32
 *    (-7.7e7 .. 1.5e8); without a resize and with PIPS_FILTER_BILINEAR everything behind the conversion is the 8-bit formats';
 *  - PIPS_FILTER_TRIANGLE with (H, W) != (h, w): the separable triangle (antialiasing) filter on the converted 8-bit planes p,
 *    PIL's and torch's antialiased bilinear in integers.  Along an axis of n source and N output samples, with m = max(n, N), the
 *    raw weight of source j for output i is r(i, j) = max(0, 2 m - |(2 j + 1) N - (2 i + 1) n|), 0 <= j < n: the triangle of
 *    half-width max(n / N, 1) around (i + 0.5) n / N, clipped to the source.  num = sum_y ry sum_x rx p and
 *    den = (sum ry)(sum rx) are exact integers, q = floor((512 num + den) / (2 den)) is the value in 8.8 fixed point rounded half
 *    up (0 <= q <= 65280); the float dst is q / 256 (exact), the uint8 dst (q + 128) >> 8 = floor(v + 0.5) of that float, so the
 *    tables agree on both outputs as above.  N == n on an axis is one tap (identity on that axis), N > n the two-tap bilinear with
 *    the clamped edge.  Within 1/512 (the rounding of q) of F.interpolate(p.double(), (H, W), mode='bilinear', antialias=True).
 *    Limits: h, w, H, W <= PIPS_FILTER_DIM_MAX and h <= 16 H, w <= 16 W -- a weight sum along an axis stays below 2^19, a row sum
 *    sum_x rx p below 2^27 (int32) and 512 num below 2^55 (int64).  With (H, W) == (h, w) no filter runs: the plain conversion.
 *    One launch: a block owns a tile of 32 x up to 8 output pixels; it stages the rows of the tile's footprint eight at a time in
 *    LDS, each source pixel converted once and read by neighbouring lanes, writes the row sums sum_x rx p (int32, one LDS plane per
 *    channel, x on the lanes) and then sums them over y in int64 and divides.  The tile's height is chosen from the ratio so that
 *    a block's LDS stays at or below 64 KiB at the 16 x limit; no workspace, no atomics, nothing outside dst written.
 *  PIPS_E_ARG from pips_frames_import_ex, ahead of any launch and with nothing written: everything pips_frames_import rejects (a
 *  format above PIPS_FMT_I010 here); an unknown filter; the filter limits; an odd plane pointer, pitch or step of a 16-bit format.
 * Known limits: chroma is replicated to its 2 x 2 pixels (nearest; chroma siting is not modelled, no bilinear chroma); the resize
 * does not antialias when it scales down unless PIPS_FILTER_TRIANGLE is asked for (the two-tap rule stays the default); the output
 * of the 10-bit formats is the 8-bit RGB of every other format (the two extra bits are not kept in the float output), BT.2020 and
 * transfer functions are not handled; dst may not overlap a source plane.
 * One launch per call: without a resize a thread owns 16 (uint8 dst) or 4 (float dst) pixels of a row, reads their source bytes
 * with 16- or 4-byte loads where the addresses allow (byte loads otherwise: the same bits for every base, pitch, step and w) and
 * stores 16 bytes per plane from the first 16-byte address of each row of dst on; with a resize a thread owns an output pixel,
 * converts its four neighbours once and fetches a chroma sample once for the neighbours that share it -- no full-size RGB
 * intermediate exists.  No atomics, no workspace, no allocation, no synchronisation; nothing outside dst is written.
 * PIPS_E_ARG ahead of any launch, with nothing written: an unknown format; an unknown matrix or range with NV12 or I420; F < 0; h,
 * w, H or W < 1; F H W > PIPS_IMPORT_PIXELS_MAX (a launch's index: split the chunk); a pitch below the bytes of a row of its
 * plane; with F > 1 a step below pitch x rows of its plane; with F > 0 a NULL dst or a NULL plane that the format has.  F = 0
 * launches nothing and returns PIPS_OK. */
#define PIPS_FMT_RGB24   0
#define PIPS_FMT_BGR24   1
#define PIPS_FMT_RGBA32  2
#define PIPS_FMT_BGRA32  3
#define PIPS_FMT_NV12    4
#define PIPS_FMT_I420    5
#define PIPS_MATRIX_BT601  0
#define PIPS_MATRIX_BT709  1
#define PIPS_RANGE_LIMITED 0
#define PIPS_RANGE_FULL    1
#define PIPS_IMPORT_PIXELS_MAX (1 << 30)
int    pips_frames_import(int format, int matrix, int range, int F, int h, int w,
                          const void* p0, size_t pitch0, size_t step0,
                          const void* p1, size_t pitch1, size_t step1,
                          const void* p2, size_t pitch2, size_t step2,
                          void* dst, int dst_is_u8, int H, int W, void* stream);
#define PIPS_FMT_P010    6
#define PIPS_FMT_I010    7
#define PIPS_FILTER_BILINEAR 0
#define PIPS_FILTER_TRIANGLE 1
#define PIPS_FILTER_DIM_MAX  8192
int    pips_frames_import_ex(int format, int matrix, int range, int filter, int F, int h, int w,
                             const void* p0, size_t pitch0, size_t step0,
                             const void* p1, size_t pitch1, size_t step1,
                             const void* p2, size_t pitch2, size_t step2,
                             void* dst, int dst_is_u8, int H, int W, void* stream);

/* Tracks out: pips_tracks_draw draws the trails of n tracks into F caller-owned surfaces of h x w IN PLACE -- the decoder's surface
 * that pips_frames_import read, on its way to an encoder or a display (chain_demo.py:92-108, utils/improc.py:655-925 draw lines
 * with a dot at the head on the CPU).  Integers only behind the quantisation of the positions:
 *  - addressing and formats: planes, pitches and steps in bytes as pips_frames_import's.  PIPS_FMT_RGB24, BGR24, RGBA32, BGRA32,
 *    NV12 and I420 are taken, and PIPS_FMT_PLANAR8: three planes R, G, B of h rows of w bytes (the (F,3,H,W) uint8 frames
 *    pips_frames_import writes: p_k = base + k H W, pitch W, step 3 H W).  Bytes outside the w x h image of a plane -- pitch
 *    padding, the alpha byte, the gap between frames -- are never written; a sample that no track covers keeps its byte and need
 *    not be written;
 *  - positions: trajs (G,n,2) float32 are pixel-index coordinates of a src_h x src_w image (the model's frames; an integer is a
 *    pixel centre), vis (G,n) logits or NULL.  Frame k of the call uses row r = first + k.  With src_w == w the x coordinate is
 *    used as it is, otherwise u = ((x + 0.5) s) - 0.5 with s = (float)w / (float)src_w, the sum, the product and the difference
 *    each rounded once to fp32 (the inverse of the import's align_corners=False resize); y likewise with h and src_h.
 *    Q = (int)floor(8 u + 0.5) (product and sum rounded once each) is the coordinate in eighths of a pixel for finite u with
 *    |u| <= 32768; for any other u (NaN, infinities, out of range), in x or in y, the point is ABSENT.  Pixel (x, y) has its
 *    centre at (8 x, 8 y) and four subsamples at (8 x +- 2, 8 y +- 2);
 *  - the primitives of track i in frame k: none when the point of row r is absent (the trail of a retired or not yet started
 *    track disappears).  Otherwise the head, a disc of radius dot8 (eighths) around the point of row r, and for every g with
 *    max(r - trail, 0) < g <= r the capsule of radius line8 around the segment from the point of row g - 1 to that of row g when
 *    both are present and |dQx| <= PIPS_DRAW_JUMP8_MAX and |dQy| <= PIPS_DRAW_JUMP8_MAX (a longer segment is a tracking failure,
 *    not a motion).  A negative radius draws nothing of its kind; trail = 0 draws heads only;
 *  - inside, in exact integers: c the subsample, P0 and P1 the ends (P0 = P1 for the disc), R the radius, a = P1 - P0,
 *    b = c - P0, L = a . a, t = a . b.  L = 0 or t <= 0: inside when b . b <= R^2; else t >= L: inside when |c - P1|^2 <= R^2;
 *    else inside when (ax by - ay bx)^2 <= R^2 L.  A subsample outside the ends' bounding box grown by R is never inside and may
 *    be skipped; within it, with |a| <= 2047 a component and R <= PIPS_DRAW_RADIUS8_MAX (16 px), a . b, b . b and the cross
 *    product stay below 2^24 (int32), the cross product's square below 2^47 and R^2 L below 2^38 (int64);
 *  - coverage: k_i in 0..4 = the subsamples of the pixel inside the UNION of track i's primitives (a joint is not drawn twice);
 *  - opacity: A_i = alpha_vis when vis == NULL or vis[r][i] > vis_logit, else alpha_occ (a NaN logit compares false); both 0..256;
 *  - blend: the tracks are applied in increasing column order i, each changing the current 8-bit value p of a sample towards
 *    its colour's component c: a full-resolution sample (R, G, B or Y) to p' = (p (1024 - k A) + c k A + 512) >> 10; a 4:2:0
 *    chroma sample, with K = the sum of k over those of its 2 x 2 pixels that lie inside the image (0..16; the edge samples of an
 *    odd h or w have fewer pixels and keep the denominator), to p' = (p (4096 - K A) + c K A + 2048) >> 12.  A weight of 0 leaves
 *    p.  The order is part of the rule: two overlapping tracks swapped give other bytes;
 *  - colours: colors (n,3) uint8 R, G, B on the device.  For NV12 and I420 each is converted once,
 *      Y = y0 + ((yr R + yg G + yb B + 32768) >> 16), Cb = clamp(128 + ((ur R + ug G + ub B + 32768) >> 16)),
 *      Cr = clamp(128 + ((vr R + vg G + vb B + 32768) >> 16)), >> the arithmetic shift, clamp to [0, 255]:
 *                                 y0  yr     yg     yb    ur      ug      ub     vr     vg      vb
 *      PIPS_MATRIX_BT601 limited  16  16829  33039  6416  -9714   -19070  28784  28784  -24103  -4681
 *      PIPS_MATRIX_BT601 full     0   19595  38470  7471  -11058  -21710  32768  32768  -27439  -5329
 *      PIPS_MATRIX_BT709 limited  16  11966  40254  4064  -6596   -22188  28784  28784  -26145  -2639
 *      PIPS_MATRIX_BT709 full     0   13933  46871  4732  -7509   -25259  32768  32768  -29763  -3005
 *    A grey gives exactly (Y, 128, 128), white 235 / 255; over all 2^24 triples every component is at most one level from
 *    floor(exact + 0.5) of the real-valued formula, limited range stays in 16..235 / 16..240, and full-range chroma reaches 256
 *    ahead of the clamp.  matrix and range are looked at for NV12 and I420 only.
 * Two launches on `stream`: one thread per (frame, track) writes a record into the workspace -- the trail + 1 quantised points, the
 * drawn segments, the box of pixels the track can touch (the boxes lie together, 16 bytes each), its opacity and converted colour; then one 256-thread block per 16 x 16
 * pixel tile and frame (it owns the tile's 8 x 8 chroma samples too) walks the tracks 256 at a time, compacts those whose box meets
 * the tile in column order (a wave ballot and a prefix over the four waves in LDS) and every thread applies them to its pixel in
 * registers; the four pixels of a chroma sample are neighbouring lanes.  A tile no track meets loads and stores nothing.  No
 * atomics, no allocation, no synchronisation; the workspace is read and written by this call only and may be reused by the next.
 * PIPS_E_ARG ahead of any launch, with nothing written: a format that is not one of the seven (PIPS_FMT_P010 and PIPS_FMT_I010
 * among them); an unknown matrix or range with NV12 or I420; F < 0; n < 0; h, w, src_h or src_w < 1; h or w > PIPS_DRAW_DIM_MAX;
 * trail outside 0..PIPS_DRAW_TRAIL_MAX; line8 or dot8 > PIPS_DRAW_RADIUS8_MAX; alpha_vis or alpha_occ outside 0..256; first < 0 or
 * first + F > G; a pitch below the bytes of a row of its plane; with F > 1 a step below pitch x rows of its plane; and with F > 0
 * and n > 0: a NULL plane that the format has, a NULL trajs, colors or workspace, a workspace off a 16-byte address, workspace_bytes <
 * pips_draw_workspace_bytes(F, n, trail) (= 4 F n (2 trail + 10) bytes; 0 for F < 0, n < 0 or a trail outside its range).  F = 0 or
 * n = 0 launches nothing and returns PIPS_OK.
 * Known limits: the 10-bit surfaces (P010, I010) are drawn on by pips_tracks_draw_ex only, and so are trails that fade with age;
 * chroma is treated as import treats it (one sample for its 2 x 2 pixels, siting not modelled); no text, one colour per track
 * (none that changes along the trail), no antialiasing beyond the four subsamples; trajs, vis, colors and the workspace may not
 * overlap a plane.
 *
 * pips_tracks_draw_ex is pips_tracks_draw with two additions; everything not named here -- positions, the quantisation to eighths,
 * the primitives, the integer inside test, opacity by visibility, column order, what is never written -- is pips_tracks_draw's
 * rule word for word (pips_tracks_draw itself is not changed and keeps rejecting formats 6 and 7):
 *  1. PIPS_FMT_P010 and PIPS_FMT_I010 beside the seven formats above.  Geometry and addressing are pips_frames_import_ex's:
 *     samples are 16-bit little-endian words, pitches and steps are in bytes, a row of Y is 2 w bytes, a row of P010's chroma
 *     2 x 2 ceil(w / 2) and of I010's 2 ceil(w / 2); every plane pointer, pitch and step must be even.  The 10-bit value v is
 *     word >> 6 for P010 and word & 1023 for I010.  A sample that gets a non-zero weight from at least one track is rewritten as
 *     v' << 6 (P010) or v' (I010): its other six bits become zero.  EVERY OTHER WORD KEEPS ALL 16 BITS -- a sample no track covers
 *     (the junk a decoder left in its unused bits included), pitch padding, the gap between frames: they are not written.  The
 *     blend is the one above on 0..1023: a full-resolution sample to (p (1024 - wgt) + c wgt + 512) >> 10, a 4:2:0 chroma sample to
 *     (p (4096 - W) + c W + 2048) >> 12; no accumulator passes 2^22.  Colours stay (n,3) uint8 R, G, B and are converted once per
 *     track, with h = 1 << (sh - 1):
 *       Y = y0 + ((yr R + yg G + yb B + h) >> sh), Cb = clamp(512 + ((ur R + ug G + ub B + h) >> sh)),
 *       Cr = clamp(512 + ((vr R + vg G + vb B + h) >> sh)), >> the arithmetic shift, clamp to [0, 1023]:
 *                                         y0  sh  yr     yg      yb     ur      ug       ub      vr      vg       vb
 *       10-bit PIPS_MATRIX_BT601 limited  64  14  16829  33039   6416   -9714   -19070   28784   28784   -24103   -4681
 *       10-bit PIPS_MATRIX_BT601 full     0   16  78612  154331  29972  -44363  -87095   131458  131458  -110079  -21379
 *       10-bit PIPS_MATRIX_BT709 limited  64  14  11966  40254   4064   -6596   -22188   28784   28784   -26145   -2639
 *       10-bit PIPS_MATRIX_BT709 full     0   16  55896  188037  18982  -30123  -101335  131458  131458  -119404  -12054
 *     The limited rows are the 8-bit constants with two more result bits: white 940, chroma within 64..960.  The full rows are the
 *     standard coefficients scaled by 65536 x 1023 / 255, rounded so that each luma row sums to 262915 and each chroma row to 0:
 *     black 0, white 1023, pure blue and red reach 1024 ahead of the clamp.  A grey gives exactly (Y, 512, 512); every component
 *     is at most one level from floor(exact + 0.5) of the real-valued formula; every accumulator stays inside int32 (< 2^27);
 *  2. fade: a HOST pointer to `trail` ints in 0..256, or NULL.  The library reads it before the launch and passes it by value; the
 *     kernels read no host memory and the array may be freed on return.  fade[a] scales the opacity of the capsule of age a: the
 *     segment that ends on the head (g = r) has age 0, the oldest age trail - 1; the head's disc always has factor 256.  Per
 *     subsample phi = the LARGEST factor among the track's primitives that contain it, 0 when none does (no order among the
 *     primitives; with a table that does not grow with age the youngest wins; a joint is still not drawn twice).  Per pixel
 *     Wp = the sum of phi over its four subsamples (0..1024) and wgt = (Wp A + 128) >> 8; for a 4:2:0 chroma sample K = the sum
 *     of Wp over its pixels inside the image (0..4096) and W = (K A + 128) >> 8.  A weight of 0 leaves the sample unwritten.  A
 *     capsule with factor 0 draws nothing.  trail = 0 reads no entry.  With fade == NULL, or with every entry 256, Wp = 256 k, so
 *     wgt = k A and W = K A exactly: THE RULE COLLAPSES TO pips_tracks_draw's, byte for byte, on the seven 8-bit formats.
 * The launches are pips_tracks_draw's: the record of a 10-bit surface holds its colour as three 10-bit fields of the same word, so
 * pips_draw_workspace_bytes serves both entries at the same size; a 2 x 2 quad is still four neighbouring lanes with 16-bit loads
 * and stores; with a table the raster blocks stage it once in LDS and keep four factors per pixel in place of the coverage mask,
 * walking the segments youngest first so that four factors of 256 end the walk.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "tracks_draw_ex:": everything pips_tracks_draw
 * rejects, except that formats 6 and 7 are legal here (an unknown matrix or range is rejected with any of the four YCbCr
 * formats); a fade entry outside 0..256; an odd plane pointer, pitch or step of a 16-bit format.  The pitch and step minimums
 * are counted in bytes of the 16-bit rows.
 * Known limits: as pips_tracks_draw's, but for the two it lifts; one colour per track (none that changes along the trail), no
 * text; BT.2020 and transfer functions are not handled, 12- and 16-bit surfaces are not taken. */
#define PIPS_FMT_PLANAR8 8
#define PIPS_DRAW_DIM_MAX     8192
#define PIPS_DRAW_TRAIL_MAX   32
#define PIPS_DRAW_RADIUS8_MAX 128
#define PIPS_DRAW_JUMP8_MAX   2047
size_t pips_draw_workspace_bytes(int F, int n, int trail);
int    pips_tracks_draw(int format, int matrix, int range, int F, int h, int w,
                        void* p0, size_t pitch0, size_t step0,
                        void* p1, size_t pitch1, size_t step1,
                        void* p2, size_t pitch2, size_t step2,
                        const float* trajs, const float* vis, int G, int n, int first, int src_h, int src_w,
                        const uint8_t* colors, int trail, int line8, int dot8, int alpha_vis, int alpha_occ, float vis_logit,
                        void* workspace, size_t workspace_bytes, void* stream);
int    pips_tracks_draw_ex(int format, int matrix, int range, int F, int h, int w,
                           void* p0, size_t pitch0, size_t step0,
                           void* p1, size_t pitch1, size_t step1,
                           void* p2, size_t pitch2, size_t step2,
                           const float* trajs, const float* vis, int G, int n, int first, int src_h, int src_w,
                           const uint8_t* colors, int trail, int line8, int dot8, int alpha_vis, int alpha_occ, float vis_logit,
                           const int* fade, void* workspace, size_t workspace_bytes, void* stream);

/* Motion: pips_motion_fit fits, for every pair of consecutive rows of trajs (F,n,2) float32 (pixel positions; vis (F,n) logits or
 * NULL), a robust 2-D similarity q = a p + t (a complex: rotation and uniform scale; t the shift) from the positions p of row f - 1
 * to the positions q of row f, 1 <= f < F: the frame-to-frame camera motion a stabiliser, an ego-motion estimate or a moving-object
 * mask starts from.  The consensus is decided in integers, 2-vectors read as complex numbers:
 *  - quantisation: s = 4 x in fp32 (exact) is the position in quarter pixels.  A row's point is USABLE when both components are
 *    finite with |s| <= PIPS_MOTION_QUARTER_MAX (8191: |x| <= 2047.75); its quantised value is rint(s), round-half-even;
 *  - valid columns: column k is VALID for pair f when it is usable in rows f - 1 and f and, with vis, vis > vis_logit holds in both
 *    rows (a NaN is not above the threshold).  The valid columns in ascending column order are the list 0..m-1;
 *  - hypotheses: K of them, 1 <= K <= PIPS_MOTION_HYPS_MAX.  Hypothesis h uses the list entries i = (mix(2h) m) >> 32 and
 *    j = (mix(2h + 1) (m - 1)) >> 32, then j += (j >= i) (64-bit products of 32-bit values).  mix(k), in 32-bit wrap-around
 *    arithmetic: u = seed + 0x9E3779B9 (g + 1) + 0x85EBCA6B (k + 1); u ^= u >> 16; u *= 0x85EBCA6B; u ^= u >> 13; u *= 0xC2B2AE35;
 *    u ^= u >> 16, with seed the 32 bits of the `seed` argument and g = frame0 + f the absolute frame index: a stream fed push by
 *    push draws the hypotheses of the whole video;
 *  - inlier test: d = p_j - p_i, e = q_j - q_i, r = e (p_k - p_i) - d (q_k - q_i) (complex products).  Column k is an inlier of h
 *    iff d != 0 and |r|^2 <= thr4^2 |d|^2, thr4 the threshold in quarter pixels, 1..PIPS_MOTION_THR4_MAX.  Every component of r is
 *    below 2^31 and both sides are below 2^62: the products of differences fit 32 bits, the two squares and the right side need 64;
 *  - selection: the score of h is its inlier count; the best hypothesis has the highest score, ties go to the lowest h.  With
 *    m < 2 or a best score below 2 the pair has NO MODEL.
 * Outputs, one row per pair (row f - 1 for pair f):
 *  - head int32[4] = (m, n_in, h_best or -1, 0);
 *  - flags uint8[n]: 0 not valid, 1 valid but outside the consensus, 2 inlier;
 *  - sums int64[8] over the inliers: n_in, S px, S py, S qx, S qy, S |p|^2, S (px qx + py qy), S (px qy - py qx) in quarter pixels
 *    (exact for n <= PIPS_MOTION_N_MAX); zeros without a model;
 *  - model float64[4] = (a_re, a_im, tx, ty), the least-squares similarity on the inliers, in pixels.  In int64, all below 2^61:
 *      D = n_in S|p|^2 - ((S px)^2 + (S py)^2),  A = n_in Sdot - (S px S qx + S py S qy),  B = n_in Scross - (S px S qy - S py S qx);
 *    then in fp64, D, A, B, the four sums and 4 n_in converted first (each rounded to nearest), one rounding per operation in this
 *    order, never fused:
 *      a_re = A / D,  a_im = B / D,  tx = (S qx - (a_re S px - a_im S py)) / (4 n_in),  ty = (S qy - (a_im S px + a_re S py)) / (4 n_in).
 *    (1, 0, 0, 0) without a model.  The model is not re-scored: the inliers are those of the winning two-point hypothesis.
 * drivers.motion_table_torch is the same rule in int64 / float64 torch ops: every output is compared bit for bit.
 * Three launches on `stream`: a 256-thread block per pair quantises the valid columns and stores them in column order (four int16
 * each; a wave ballot and a prefix over the waves, no atomics); a block per (pair, 64 hypotheses) scores them -- a lane owns a
 * hypothesis, the points pass through LDS in tiles of 2048 (n is not limited by LDS) and the block stores its best (score, h) with
 * a plain store; a block per pair picks the winner, tests every column against it and writes flags, sums, head and model.  No
 * atomics, no allocation, no synchronisation; the workspace is read and written by this call only.
 * pips_motion_workspace_bytes(F, n, K) = (F - 1) (8 n + 4 (1 + ceil(K / 64))); 0 for F <= 1, n <= 0 or arguments pips_motion_fit
 * rejects.  PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "motion_fit:": F < 0 or >
 * PIPS_MOTION_ROWS_MAX; n < 0 or > PIPS_MOTION_N_MAX; K outside 1..PIPS_MOTION_HYPS_MAX; thr4 outside 1..PIPS_MOTION_THR4_MAX;
 * frame0 < 0 or frame0 + F > INT_MAX; a NaN vis_logit; with F > 1 a NULL head, sums or model; with F > 1 and n > 0 a NULL trajs,
 * flags or workspace or a workspace off a 16-byte address.  PIPS_E_WORKSPACE: workspace_bytes < pips_motion_workspace_bytes(F, n, K).
 * F <= 1 launches nothing, writes nothing and returns PIPS_OK.  n == 0 with F > 1 needs no workspace and runs the last launch alone:
 * every head row is (0, 0, -1, 0), sums are zeros and the model is the identity.
 * Known limits: a similarity only (no affine, no homography, no rolling shutter); no re-scoring after the refit; the frames are
 * not warped and the cover step does not use the result. */
#define PIPS_MOTION_QUARTER_MAX 8191
#define PIPS_MOTION_HYPS_MAX    1024
#define PIPS_MOTION_THR4_MAX    1024
#define PIPS_MOTION_N_MAX       65536
#define PIPS_MOTION_ROWS_MAX    (1 << 24)
size_t pips_motion_workspace_bytes(int F, int n, int K);
int    pips_motion_fit(const float* trajs, const float* vis, int F, int n, int frame0, float vis_logit, int K, int thr4, int seed,
                       int32_t* head, int64_t* sums, double* model, uint8_t* flags, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Motion layers: pips_motion_layers answers WHAT moves.  For every pair of consecutive rows it finds the camera's similarity as
 * pips_motion_fit does, then repeats the consensus on the columns left over, for L layers, and counts how the layers of a pair
 * overlap those of the pair before, so that a host can link them into objects that persist (drivers.link_layers).  Everything not
 * restated here is pips_motion_fit's rule above, word for word: quantisation, usable and valid columns, mix, the choice of i and j,
 * the inlier test, the key score * 1024 + (1023 - h), ties to the lowest h, the eight sums and the fp64 model with one rounding per
 * operation.  Per pair f (1 <= f < F) and layer l = 0..L-1, in this order:
 *  - the LIST of layer l holds the valid columns of the pair that no layer below l took, in ascending column order; m_l its length;
 *  - layer l draws its hypotheses with seed_l = seed + l * 0x632BE5AB (32-bit wrap-around) in place of seed: seed_0 = seed, layer 0
 *    draws pips_motion_fit's hypotheses.  The indices i and j index layer l's own list, with m_l in place of m;
 *  - layer l HAS A MODEL iff m_l >= 2 and its best score is at least need_l: need_0 = 2 as pips_motion_fit, need_l = min_in for
 *    l >= 1, 2 <= min_in <= PIPS_MOTION_N_MAX;
 *  - with a model the inliers of the winning hypothesis leave the list.  Without a model nothing leaves, and the next layer is
 *    still tried on the same columns with its own hypotheses: there is no early stop, every layer follows one rule.
 * Outputs, one row per pair (row f - 1 for pair f), 1 <= L <= PIPS_MOTION_LAYERS_MAX:
 *  - layer uint8[n]: 255 for a column that is not valid, 254 for a valid column in no layer, otherwise the l that took the column;
 *  - per (pair, layer), row (f - 1) L + l: head int32[4] = (m_l, n_in, h_best or -1, 0); sums int64[8] and model float64[4],
 *    pips_motion_fit's formulas on that layer's inliers (zeros and (1, 0, 0, 0) without a model); box int32[4] = (min qx, min qy,
 *    max qx, max qy) of the inliers' positions in row f, in quarter pixels (zeros without a model);
 *  - overlap int32[L][L] per pair: overlap[a][b] is the number of columns k with layer_f[k] == a and prev[k] == b, for a, b < L
 *    (254 and 255 on either side count nowhere).  prev is the pair before, layer_{f-1}; for the first pair of a call it is
 *    prev_layer uint8[n], the labels of the pair before this call in THIS call's column order, or NULL: then the first pair's table
 *    is all zeros.  prev_layer may NOT lie inside this call's `layer` output (its first launch writes every row of `layer` before
 *    the last one reads prev_layer): a host that keeps the last row of one call for the next copies it out of the buffer first.
 * Layer 0 is pips_motion_fit: head, sums and model of layer 0 are its rows, layer == 0 where its flags are 2 and layer == 255 where
 * they are 0.  drivers.motion_layers_table_torch is the same rule in int64 / float64 torch ops: every output is compared bit for bit.
 * 1 + 2 L + 1 launches on `stream`, no atomics: a block per pair quantises the valid columns once and stores them in column order
 * (four int16 and the int32 column index each) and writes 255 / 254 into layer; per layer, pips_motion_fit's scoring launch on the
 * layer's list with seed_l, then a block per pair that picks the winner, tests the list's entries, writes layer[col] = l and the
 * (pair, layer) rows and compacts the entries that stay into the other of two ping-pong lists (a wave ballot and a prefix over the
 * waves: stable); a last block per pair counts the L * L (now, before) codes with one ballot a code.  A pair whose list is shorter
 * than 2 costs its scoring blocks one load and its select block the copy of at most one entry.
 * pips_motion_layers_workspace_bytes(F, n, K, L) = (F - 1) (24 n + 4 (1 + ceil(K / 64))), whatever L; 0 for F <= 1, n <= 0 or
 * arguments pips_motion_layers rejects.  PIPS_E_ARG ahead of any launch, with nothing written and the message prefix
 * "motion_layers:": pips_motion_fit's rejections of F, n, K, thr4, frame0 and vis_logit; L outside 1..PIPS_MOTION_LAYERS_MAX; min_in
 * outside 2..PIPS_MOTION_N_MAX; with F > 1 a NULL head, sums, model, box or overlap; with F > 1 and n > 0 a NULL trajs, layer or
 * workspace, a workspace off a 16-byte address or a prev_layer whose n bytes meet the (F - 1) n bytes of layer.
 * PIPS_E_WORKSPACE: workspace_bytes below the figure above.  F <= 1 launches
 * nothing, writes nothing and returns PIPS_OK.  n == 0 with F > 1 needs no workspace: every head row is (0, 0, -1, 0), sums, box and
 * overlap are zeros and every model is the identity.
 * Known limits: similarities only (no affine or homography layers); a layer is a motion, not a region -- nothing makes it spatially
 * compact; no re-scoring after the refit; layers whose motions coincide are not merged; the overlap table links a pair to the pair
 * before and no further, so an identity linked from it has no memory beyond one pair; labels are per track (pips_object_masks
 * below makes the per-pixel masks). */
#define PIPS_MOTION_LAYERS_MAX  8
size_t pips_motion_layers_workspace_bytes(int F, int n, int K, int L);
int    pips_motion_layers(const float* trajs, const float* vis, const uint8_t* prev_layer, int F, int n, int frame0, float vis_logit,
                          int K, int thr4, int seed, int L, int min_in, int32_t* head, int64_t* sums, double* model, int32_t* box,
                          uint8_t* layer, int32_t* overlap, void* workspace, size_t workspace_bytes, void* stream);

/* Object masks: pips_object_masks turns a label per TRACK (pips_motion_layers' `layer` rows, or any uint8 labels) into a label per
 * PIXEL of an h x w image: every pixel takes the label its nearest tracks vote for.  Integers only behind the quantisation:
 *  - positions: frame k of the call uses row r = first + k of trajs (G,n,2) float32 and of labels (G,n) uint8.  A position becomes
 *    Q, in eighths of a pixel of the h x w mask, by pips_tracks_draw's rule above, word for word (the same device function): the
 *    scaling from src_h x src_w when the sizes differ, one rounding per operation, Q = floor(8 u + 0.5), and the point is ABSENT for
 *    NaN, infinities and |u| > 32768 in x or in y.  Pixel (X, Y) has its centre at (8 X, 8 Y);
 *  - who takes part: column i takes part in frame k when its point of row r is present and labels[r][i] != PIPS_MASK_NONE (255);
 *  - candidates of a pixel: the participating columns with dx = 8 X - Qx, dy = 8 Y - Qy, |dx| <= radius8, |dy| <= radius8 and
 *    d2 = dx^2 + dy^2 <= radius8^2 (a column at exactly the radius is in);
 *  - order: candidates are ordered by the key (d2, column): of two candidates at the same distance the lower column is nearer;
 *  - vote: the min(vote, candidates) nearest candidates vote, one each, for their label; the pixel gets the label with the most
 *    votes, and among labels with equally many the one that holds the smallest key;
 *  - a pixel with no candidate gets PIPS_MASK_NONE;
 *  - what is written: every byte of the w x h image of every frame, frame k at mask + k step, row Y at + Y pitch (bytes).  Pitch
 *    padding and the gap between frames are never written.
 * Limits: radius8 in 0..PIPS_MASK_RADIUS8_MAX (256 px), vote in 1..PIPS_MASK_VOTE_MAX, n <= PIPS_MASK_N_MAX, h and w <=
 * PIPS_DRAW_DIM_MAX.  With these d2 <= 2^22 and the key d2 2^24 + column 2^8 + label fits an int64 (below 2^48).
 * drivers.object_masks_torch is the same rule in int64 torch ops: every byte is compared.
 * Two launches on `stream`: one thread per (frame, column) writes an 8-byte record into the workspace -- Qx, and Qy 2^8 + label
 * (|Q| < 2^19), or ABSENT for a column that takes no part; then one 256-thread block per 32 x 32 pixel tile and frame walks the
 * records 256 at a time, compacts those within radius8 of the tile in column order (a wave ballot and a prefix over the four
 * waves in LDS) and every thread keeps the `vote` smallest keys of its four neighbouring pixels of a row in registers; it stores
 * them as one dword where the address allows.  No atomics, no allocation, no synchronisation; the workspace is read and written by
 * this call only and may be reused by the next.
 * pips_object_masks_workspace_bytes(F, n) = 8 F n; 0 for F < 0, n < 0 or n > PIPS_MASK_N_MAX.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "object_masks:": F < 0, n < 0 or G < 0; n >
 * PIPS_MASK_N_MAX; h, w, src_h or src_w < 1; h or w > PIPS_DRAW_DIM_MAX; radius8 or vote outside its range; first < 0 or first + F >
 * G; pitch < w; with F > 1 a step below pitch x h; with F > 0 a NULL mask; with F > 0 and n > 0 a NULL trajs, labels or workspace,
 * workspace_bytes below the figure above, a workspace off a 16-byte address.  F = 0 launches nothing and returns PIPS_OK; n = 0
 * needs no trajs, labels or workspace and fills the images with PIPS_MASK_NONE.
 *
 * pips_masks_tint shows such a label plane on F caller-owned surfaces of h x w IN PLACE: a colour and an opacity per (frame,
 * label).  Formats, planes, pitches and steps are pips_tracks_draw's: the seven 8-bit formats RGB24, BGR24, RGBA32, BGRA32, NV12,
 * I420 and PLANAR8.  mask: frame k at mask + k mask_step, row Y at + Y mask_pitch, a byte a pixel (the surface's own size).
 * colors (F,C,3) uint8 R G B on the DEVICE; alpha (F,C) int in 0..256 on the HOST -- the library reads it before the launch and
 * passes it by value, so it can be checked and may be freed on return; 1 <= C <= PIPS_MASK_LABELS_MAX.
 *  - a pixel of frame f whose label l < C has the opacity A = alpha[f][l] and the colour colors[f][l], for NV12 and I420 converted
 *    once to Y Cb Cr by pips_tracks_draw's 8-bit table (matrix and range are looked at for these two only); a label >= C has
 *    A = 0 (PIPS_MASK_NONE is such a label);
 *  - a full-resolution sample (R, G, B or Y) goes to p' = (p (256 - A) + c A + 128) >> 8;
 *  - a 4:2:0 chroma sample, the sums running over those of its 2 x 2 pixels j that lie inside the image, goes to
 *    p' = (p (1024 - S A_j) + S c_j A_j + 512) >> 10 (the edge samples of an odd h or w keep the denominator, as in draw);
 *  - a weight of 0 leaves the sample as it is.  The alpha byte of RGBA32 / BGRA32, pitch padding and gaps are never written.
 * drivers.tint_masks_torch is the same rule in int64 torch ops: every byte is compared.
 * One launch per floor(1024 / C) frames on `stream` (1024 opacities travel in a launch's arguments: one launch for 128 frames of
 * 8 labels), no workspace: a 256-thread block per 64 x 32 pixel tile and frame first converts the frame's C (opacity, colour) pairs
 * into LDS; a thread owns 4 x 2 pixels and their two chroma samples, reads its labels as dwords and, where any has a weight, the
 * samples as dwords where the address allows; four samples that the blend leaves as they were are not stored, so a tile whose
 * labels all have weight 0 touches no surface byte.  No atomics, no allocation, no synchronisation.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "masks_tint:": a format that is not one of the seven
 * (P010 and I010 among them); an unknown matrix or range with NV12 or I420; F < 0; h or w < 1 or > PIPS_DRAW_DIM_MAX; C outside
 * 1..PIPS_MASK_LABELS_MAX; a pitch below the bytes of a row of its plane or of the mask; with F > 1 a step below pitch x rows; and
 * with F > 0: a NULL plane that the format has, a NULL mask, colors or alpha, an alpha entry outside 0..256.  F = 0 launches nothing.
 * Known limits: in pips_object_masks the nearest tracks decide, not the image (pips_object_masks_guided below lets the image's
 * luma edges decide; no colour distances, no smoothing of the guide); no tint on P010 / I010; no outlines, no text; a mask is made
 * from one row alone (no temporal smoothing); mask and surface have one size; the mask, colors and the workspace may not overlap a
 * plane. */
#define PIPS_MASK_NONE        255
#define PIPS_MASK_RADIUS8_MAX 2048
#define PIPS_MASK_VOTE_MAX    5
#define PIPS_MASK_N_MAX       65536
#define PIPS_MASK_LABELS_MAX  255
size_t pips_object_masks_workspace_bytes(int F, int n);
int    pips_object_masks(const float* trajs, const uint8_t* labels, int G, int n, int first, int F,
                         int src_h, int src_w, int h, int w, int radius8, int vote,
                         uint8_t* mask, size_t pitch, size_t step,
                         void* workspace, size_t workspace_bytes, void* stream);
int    pips_masks_tint(int format, int matrix, int range, int F, int h, int w,
                       void* p0, size_t pitch0, size_t step0,
                       void* p1, size_t pitch1, size_t step1,
                       void* p2, size_t pitch2, size_t step2,
                       const uint8_t* mask, size_t mask_pitch, size_t mask_step,
                       const uint8_t* colors, const int* alpha, int C, void* stream);

/* Object masks that follow image edges: pips_object_masks_guided makes the same label plane as pips_object_masks, but a pixel
 * takes the label of the track that is nearest ALONG A PATH that avoids crossing luma edges -- a geodesic distance on an 8-bit
 * guide plane of the mask's size (the surface's own luma) -- so the boundary between two labels runs along the object's outline
 * where the image shows one, not halfway between two tracks.  Integers only behind the quantisation.  Per frame k of the call,
 * row r = first + k:
 *  - positions and who takes part: exactly pips_object_masks' rules -- Q in eighths of a pixel of the h x w mask by
 *    pips_tracks_draw's quantisation (the same device function); column i takes part when its point is present and
 *    labels[r][i] != PIPS_MASK_NONE;
 *  - seeds: a participating column seeds the pixel X = (Qx + 4) >> 3, Y = (Qy + 4) >> 3 (arithmetic shift).  A seed pixel outside
 *    the image seeds nothing;
 *  - state: one 32-bit key per pixel, cost << 16 | column, or 0xFFFFFFFF for none.  A seed pixel starts with cost 0 and the
 *    lowest column that seeds it; every other pixel starts as none;
 *  - step cost: the step between 8-neighbours p and q, both inside the image, costs c(p,q) = L + edge |G(p) - G(q)|, L = 5 for
 *    the four axial neighbours and L = 7 for the four diagonal ones (the 5-7 chamfer), G the guide plane: frame k at guide + k
 *    guide_step, row Y at + Y guide_pitch, a byte a pixel;
 *  - relaxation: key'(p) = min(key(p), min over the neighbours q that have a key and cost(q) + c(p,q) <= reach of
 *    (cost(q) + c(p,q)) << 16 | column(q));
 *  - result: the fixed point of that relaxation.  Every step costs at least 5, so a path within `reach` has at most
 *    floor(reach / 5) steps and that many Jacobi applications from the seeds reach the fixed point; it equals Dijkstra on the
 *    keys -- cost first, then the lower column;
 *  - output: mask[Y][X] = labels[r][column] of the pixel's key, PIPS_MASK_NONE where it has none.  Every byte of the w x h image
 *    of every frame is written; pitch padding and the gap between frames are never written.
 * Limits: edge in 0..PIPS_MASK_EDGE_MAX, reach in 0..PIPS_MASK_REACH_MAX, n <= PIPS_MASK_N_MAX, h and w <= PIPS_DRAW_DIM_MAX.
 * With these c <= 16327 and cost + c <= 49094: a key never wraps and never collides with none.  edge = 0 is the chamfer Voronoi
 * diagram of the seed pixels cut off at reach / 5 px.  drivers.object_masks_guided_torch is the same rule in int64 torch ops: every
 * byte is compared.
 * Launches on `stream`: one thread per (frame, column) writes an 8-byte record into the workspace -- the seed pixel Y << 16 | X,
 * or -1, and the label -- then ceil(floor(reach / 5) / 16) launches, at least one, counted on the host from `reach` alone: no
 * convergence flag comes back from the device.  In each a 256-thread block owns a 64 x 64 pixel tile of one frame, holds the keys
 * and the guide of the tile grown by 16 pixels a side in LDS, relaxes them there -- 16 in-place sweeps over the four classes
 * (X & 1, Y & 1) of pixels, a barrier between two classes, leaving early when a sweep changes nothing -- and stores the tile
 * alone.  The first launch builds the seeds of its patch from the records (an integer atomicMin in LDS: the lowest column), the
 * launches hand the keys on through two planes in the workspace in turn, the last gathers the labels and stores them as dwords
 * where the address allows.  The schedule does at least the Jacobi steps and never below the fixed point; the relaxation is
 * monotone, so the result is the fixed point and a pure function of the inputs.  No other atomics, no allocation, no
 * synchronisation; the workspace is read and written by this call only and may be reused by the next.
 * pips_object_masks_guided_workspace_bytes(F, n, h, w) = (8 F n rounded up to 16) + 2 x 4 F h w: the records and two key planes;
 * 0 for F = 0 or n = 0 and for F < 0, n < 0, n > PIPS_MASK_N_MAX, h or w < 1 or > PIPS_DRAW_DIM_MAX.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "object_masks_guided:": F < 0, n < 0 or G < 0; n >
 * PIPS_MASK_N_MAX; h, w, src_h or src_w < 1; h or w > PIPS_DRAW_DIM_MAX; edge or reach outside its range; first < 0 or first + F >
 * G; pitch < w; with F > 1 a step below pitch x h; with F > 0 a NULL mask; with F > 0 and n > 0 a NULL trajs, labels, guide or
 * workspace, guide_pitch < w, with F > 1 a guide_step below guide_pitch x h, workspace_bytes below the figure above, a workspace
 * off a 16-byte address.  F = 0 launches nothing and returns PIPS_OK; n = 0 needs no trajs, labels, guide or workspace and fills
 * the images with PIPS_MASK_NONE in one launch.
 *
 * pips_guide_plane makes such a guide from F surfaces of h x w: G = (77 R + 150 G + 29 B + 128) >> 8, the luma of
 * pips_corner_table and pips_cut_table, for the formats RGB24, BGR24, RGBA32, BGRA32 (plane 0) and PLANAR8 (planes 0, 1, 2 = R, G,
 * B); planes, pitches and steps in bytes as in pips_tracks_draw.  One launch on `stream`: a thread per four neighbouring pixels
 * of a row, a dword store where the address allows; frames past the 65535th are walked by the same blocks.  The Y plane of an
 * NV12 or I420 surface IS a guide and goes into pips_object_masks_guided by pointer, pitch and step without a copy.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "guide_plane:": any other format (NV12, I420, P010
 * and I010 among them); F < 0; h or w < 1 or > PIPS_DRAW_DIM_MAX; a pitch below the bytes of a row of its plane or guide_pitch <
 * w; with F > 1 a step below pitch x h; with F > 0 a NULL plane that the format has or a NULL guide.  F = 0 launches nothing.
 * Known limits: luma only (no colour distances), 8-bit guides only, no smoothing or denoising of the guide, one geodesic
 * neighbour decides (no vote), no temporal smoothing; every first-launch block walks all n records (they are not binned by
 * tile); the guide, the mask and the workspace may not overlap. */
#define PIPS_MASK_EDGE_MAX    64
#define PIPS_MASK_REACH_MAX   32767
size_t pips_object_masks_guided_workspace_bytes(int F, int n, int h, int w);
int    pips_object_masks_guided(const float* trajs, const uint8_t* labels, int G, int n, int first, int F,
                                int src_h, int src_w, int h, int w, int edge, int reach,
                                const uint8_t* guide, size_t guide_pitch, size_t guide_step,
                                uint8_t* mask, size_t pitch, size_t step,
                                void* workspace, size_t workspace_bytes, void* stream);
int    pips_guide_plane(int format, int F, int h, int w,
                        const void* p0, size_t pitch0, size_t step0,
                        const void* p1, size_t pitch1, size_t step1,
                        const void* p2, size_t pitch2, size_t step2,
                        uint8_t* guide, size_t guide_pitch, size_t guide_step, void* stream);

/* Frames out, stabilised: pips_frames_warp resamples F frames from the `src` surfaces into the `dst` surfaces, format and size the
 * same on both sides, through one affine map per frame -- what a stabiliser does with pips_motion_fit's models
 * (drivers.motion_path, drivers.motion_smooth, drivers.warp_coefficients make the coefficients on the host).  Integers only:
 *  - formats and addressing: all nine formats, PIPS_FMT_RGB24, BGR24, RGBA32, BGRA32, NV12, I420, P010, I010 and PLANAR8.  Planes,
 *    pitches and steps in bytes, the plane geometry (odd h and w legal, chroma planes of ceil(h/2) x ceil(w/2) samples) and the
 *    even pointers, pitches and steps of the 16-bit formats are pips_tracks_draw_ex's.  src is const.  NO PLANE OF dst MAY OVERLAP A
 *    PLANE OF src: the byte range of plane k is [p_k, p_k + (F - 1) step_k + (rows_k - 1) pitch_k + the bytes of a row), and an
 *    intersection of a src range with a dst range is rejected;
 *  - coefficients: coef (F,6) int32 on the device.  Row f = (m0, m1, m2, m3, m4, m5) maps OUTPUT pixel indices to SOURCE positions;
 *    m0, m1, m3, m4 are in Q24 (2^24 = 1.0), m2 and m5 in Q16 pixels;
 *  - position of a full-resolution sample (R, G, B of a pixel, Y) at output pixel (x, y): X = m0 x + m1 y + 256 m2 in int64,
 *    U = (X + 32768) >> 16 with the arithmetic shift: the source x in 1/256 px, rounded half up.  x0 = U >> 8, fx = U & 255; V, y0
 *    and fy likewise from m3, m4, m5.  Tap indices are compared with the image bounds as int64 before any narrowing: coefficients
 *    at INT32_MIN / INT32_MAX are legal and land outside;
 *  - position of a 4:2:0 chroma sample (cx, cy), which stands at luma position (2 cx + 0.5, 2 cy + 0.5) (siting is not modelled,
 *    as in import and draw): XL = m0 (4 cx + 1) + m1 (4 cy + 1) + 512 m2, Uc = (XL - 2^24 + 2^17) >> 18 is the position in the
 *    chroma grid in 1/256 sample, Vc likewise; the identity gives Uc = 256 cx.  Cb and Cr share taps and weights;
 *  - value: with p00, p01, p10, p11 the taps at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1),
 *      v = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16
 *    (below 2^27 for 10-bit samples: int32).  A 10-bit sample is read as draw reads it (word >> 6 for P010, word & 1023 for I010)
 *    and written as v << 6 (P010) or v (I010); EVERY word of dst inside the image is written.  The alpha byte of RGBA32 / BGRA32
 *    dst is written 255 (src's is not read).  Bytes outside the w x h image of a plane are never written;
 *  - border: PIPS_WARP_BORDER_CONSTANT -- a tap outside the plane takes the fill value; PIPS_WARP_BORDER_REPLICATE -- a tap's index
 *    is clamped into the plane.  fill_rgb is one int 0xRRGGBB: the RGB formats use its bytes, NV12 / I420 convert it once by
 *    pips_tracks_draw's table and P010 / I010 by pips_tracks_draw_ex's 10-bit table (matrix and range are looked at for these four
 *    only).  A tap with weight 0 contributes nothing, so the identity (2^24, 0, 0, 0, 2^24, 0) copies every sample exactly, the last
 *    row and column included, under either border.
 * drivers.warp_frames_torch is the same rule in int64 torch ops: every byte is compared.
 * One launch on `stream`: a 256-thread block owns a 64 x 16 tile of output luma of one frame and that tile's 32 x 8 chroma samples;
 * a thread produces two or four adjacent samples of a row (whole dwords) and stores dwords where the dst address allows.  The block computes the box of
 * source samples its tile can tap from the same integers at the tile's four corners, the +1 tap added; when that box, with rows
 * of round_up(width x bytes of a pixel + 3, 4) bytes, is at most 12288 bytes in every plane, its rows are staged in LDS (aligned
 * dword loads, byte loads at the ragged ends) and the taps read there, otherwise the taps are read from global memory: the same
 * bits either way, and the choice depends on the coefficients, the format and the tile alone.  A tile whose box lies inside the
 * plane takes the same pass without the border rule (no tap can be outside).  No workspace, no atomics, no
 * allocation, no synchronisation, no floating point.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "frames_warp:": an unknown format or border; an
 * unknown matrix or range with a YCbCr format; fill_rgb outside 0..0xFFFFFF; F < 0; h or w < 1 or > PIPS_WARP_DIM_MAX; a pitch
 * below the bytes of a row of its plane; with F > 1 a step below pitch x rows of its plane; an odd plane pointer, pitch or step of
 * a 16-bit format; and with F > 0: a NULL plane that the format has, a NULL coef, src and dst ranges that overlap.  F = 0 launches
 * nothing and returns PIPS_OK.
 * Known limits: bilinear only (no bicubic, no Lanczos, no antialiasing when the map shrinks the image); chroma siting is not
 * modelled; the single-pixel chroma samples of an odd edge are treated like any other; alpha is not resampled; an affine map only
 * (no homography, no rolling shutter). */
#define PIPS_WARP_BORDER_CONSTANT  0
#define PIPS_WARP_BORDER_REPLICATE 1
#define PIPS_WARP_DIM_MAX 8192
int    pips_frames_warp(int format, int matrix, int range, int border, int fill_rgb, int F, int h, int w,
                        const void* s0, size_t spitch0, size_t sstep0,
                        const void* s1, size_t spitch1, size_t sstep1,
                        const void* s2, size_t spitch2, size_t sstep2,
                        void* d0, size_t dpitch0, size_t dstep0,
                        void* d1, size_t dpitch1, size_t dstep1,
                        void* d2, size_t dpitch2, size_t dstep2,
                        const int32_t* coef, void* stream);

/* The border of a stabilised frame filled from neighbouring frames: pips_frames_warp_fill writes Fd output frames from Fs source
 * frames, format and h x w the same on both sides.  Output frame j has K candidates, 1 <= K <= PIPS_WARP_FILL_MAX: cand (Fd,K)
 * int32 on the device, cand[j][k] an index into the source frames, and coef (Fd,K,6) int32 on the device, coef[j][k] a row of
 * exactly pips_frames_warp's meaning and fixed point.  The decision is made for every output sample of every plane on its own:
 *  1. position: U, V of candidate k are pips_frames_warp's, in int64 -- luma U = (X + 32768) >> 16, chroma
 *     Uc = (XL - 2^24 + 2^17) >> 18 -- and x0 = U >> 8, fx = U & 255, y0 = V >> 8, fy = V & 255;
 *  2. valid: candidate k is valid when 0 <= cand[j][k] < Fs.  An invalid candidate is skipped; -1 is the conventional "none";
 *  3. covers: a valid candidate covers the sample when every tap that has weight lies inside the plane, pw x ph the sample grid of
 *     that plane: x0 >= 0 and (x0 + 1 <= pw - 1, or fx == 0 and x0 <= pw - 1) on the x axis, and the same with y0, fy, ph on the
 *     y axis.  The identity therefore covers every sample, the last row and column included;
 *  4. value: the plain two-by-two blend of pips_frames_warp (no border rule needed) from the first candidate in list order that
 *     covers the sample, read from source frame cand[j][k].  If none covers it: pips_frames_warp's value for candidate 0 under
 *     border / fill_rgb, partial taps blended with the fill or clamped exactly as there; if candidate 0 is itself invalid, the
 *     fill value, whatever border is.  K = 1 with cand[j][0] = j is pips_frames_warp, byte for byte;
 *  5. source map: `source` is NULL or an (Fd,h,w) uint8 surface with its own pitch and step in bytes.  It receives, for plane 0,
 *     the list position k that supplied the sample, or 255 where none covered.  The three planes of PLANAR8 share positions, so
 *     plane 0 speaks for them;
 *  6. unchanged from pips_frames_warp: formats and addressing, the 10-bit read and write, the alpha byte (written 255), every word
 *     of dst inside the image is written, nothing outside the image is written and nothing outside a src plane is read.  cand and
 *     coef are not read back to the host.
 * drivers.warp_frames_fill_torch is the same rule in int64 torch ops: every byte is compared, the source map included.
 * One launch on `stream` per 65535 output frames: pips_frames_warp's block per 64 x 16 luma tile and OUTPUT frame.  A tile whose
 * candidate-0 box lies inside every plane, candidate 0 valid, cannot have an uncovered sample: it runs pips_frames_warp's staged
 * or direct pass on frame cand[j][0] and writes zeros to the source map.  Every other tile walks the list: a thread keeps a
 * done-mask over its two or four samples in registers, skips (with its whole block) an invalid candidate and one whose box misses
 * the plane, leaves the list when nothing of it is left to fill, and takes the rule-4 fallback at the end; these tiles read
 * their taps from global memory.  No workspace, no atomics, no allocation, no synchronisation, no floating point; dword stores
 * where the address allows, the source map too.
 * PIPS_E_ARG ahead of any launch, with nothing written and the message prefix "frames_warp_fill:": everything pips_frames_warp
 * rejects, applied to Fs with src and to Fd with dst separately; K outside 1..PIPS_WARP_FILL_MAX; with Fd > 0 a NULL cand or coef, a
 * NULL dst plane, and with Fs > 0 a NULL src plane; a source pitch below w, or with Fd > 1 a source step below pitch x h; dst or
 * source overlapping src or each other.  Fd = 0 launches nothing and returns PIPS_OK.
 * Known limits beside pips_frames_warp's: a moving object is shown where the neighbour saw it (ghosts in the border); no
 * feathering and no exposure matching at the seam; luma and chroma choose their candidate independently, so a one-sample fringe
 * is possible on a seam; nothing comes from frames outside the list. */
#define PIPS_WARP_FILL_MAX 16
int    pips_frames_warp_fill(int format, int matrix, int range, int border, int fill_rgb, int Fs, int Fd, int K, int h, int w,
                             const void* s0, size_t spitch0, size_t sstep0,
                             const void* s1, size_t spitch1, size_t sstep1,
                             const void* s2, size_t spitch2, size_t sstep2,
                             void* d0, size_t dpitch0, size_t dstep0,
                             void* d1, size_t dpitch1, size_t dstep1,
                             void* d2, size_t dpitch2, size_t dstep2,
                             const int32_t* cand, const int32_t* coef,
                             uint8_t* source, size_t source_pitch, size_t source_step, void* stream);

/* utils.samp.bilinear_sample2d (utils/samp.py:5-78): clamped-index point sample of frame
 * 0 of every clip.  xy (B,N,2) in map pixels -> out (B,N,128).  PIPS_E_ARG ahead of the launch for a
 * NULL pointer or B, S, N, H8 or W8 below 1. */
int    pips_point_sample(const float* level0, int B, int S, int H8, int W8,
                         const float* xy, int N, float* out, void* stream);

/* CorrBlock.corr + CorrBlock.sample + get_3d_embedding + the concat of
 * DeltaBlock.forward (nets/pips.py:384-398, 355-382, 517-522, 304-308; utils/misc.py:44-69):
 * builds the mixer input X (B*N*S, 544) = [ffeat 128 | corr 196 | sincos 192 | dx dy t | 0..].
 * ffeats (B*N*S,128), coords (B*N*S,2) in map pixels, both particle-major.  H8, W8 >= 16 in every form below (the map size rule
 * at pips_forward: PIPS_E_ARG ahead of any launch otherwise).  Finite coordinates of any size are defined: a window wholly outside
 * the map gives 196 zeros. */
int    pips_mixer_input_build(const float* pyramid, int B, int S, int H8, int W8,
                              const float* ffeats, const float* coords, const float* times,
                              int N, float* X, void* stream);
/* the same with per-particle window starts (pips_track's win_start, may be NULL) and flags = 0 | PIPS_FLAG_BF16_MAPS */
int    pips_mixer_input_build_ex(const float* pyramid, int B, int S, int H8, int W8, const float* ffeats, const float* coords,
                                 const float* times, int N, const int* win_start, int flags, float* X, void* stream);
/* pips_mixer_input_build_ex plus pips_track_win's win_dir and the window length S (1..PIPS_S_MAX; rows of ffeats / coords / X
 * are B*N*S); T = frames per clip in the pyramid */
int    pips_mixer_input_build_win(const float* pyramid, int B, int T, int H8, int W8, const float* ffeats, const float* coords,
                                  const float* times, int N, const int* win_start, const int* win_dir, int flags, int S,
                                  float* X, void* stream);
/* pips_mixer_input_build_win on a ring of R frame slots per clip holding T logical frames (pips_track_ring) */
int    pips_mixer_input_build_ring(const float* pyramid, int B, int T, int R, int H8, int W8, const float* ffeats,
                                   const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                   int flags, int S, float* X, void* stream);
/* pips_mixer_input_build_ring with the clip table of pips_track_clips (win_clip = NULL: exactly pips_mixer_input_build_ring) */
int    pips_mixer_input_build_clips(const float* pyramid, int B, int T, int R, int H8, int W8, const float* ffeats,
                                    const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                    const int* win_clip, const int* clip_first, const int* clip_frames, int V,
                                    int flags, int S, float* X, void* stream);
/* the gather of pips_track_rings: V rings of R slots on a pyramid laid out for F slots (checks as pips_track_rings) */
int    pips_mixer_input_build_rings(const float* pyramid, int B, int F, int R, int H8, int W8, const float* ffeats,
                                    const float* coords, const float* times, int N, const int* win_start, const int* win_dir,
                                    const int* win_clip, const int* clip_first, const int* clip_frames, int V,
                                    int flags, int S, float* X, void* stream);

/* Same result as pips_mixer_input_build through the LDS-tiled kernels meant for dense query sets
 * (BASELINE configs[3], test_on_davis.py:103-130): particles binned by 16x16 map tile, the tile's
 * halo region at each level staged in LDS once per tile (csrc/gather_tiled.hip).  pips_track /
 * pips_forward pick it by themselves when the query set is dense (>= 16 particles per tile on average and >= 1024 per
 * frame -- >= 256 with PIPS_FLAG_BF16_MAPS, whose matrix-core kernel pays earlier: BASELINE configs[2] takes it since
 * round 6 -- within the kernel's 32-bit offset limits; otherwise the direct kernel).  scratch holds the per-frame sort,
 * the per-tile tables and (read by the bf16 mode's kernel) the features as bf16 in the sorted order; values agree
 * with the direct kernel to fp32 summation order.  The _timed form also returns the HIP-event
 * durations (ms) of its three launches {bin_particles, embed_rows, gather_tiled} in ms3_host and
 * synchronises the stream (measurement only). */
size_t pips_gather_scratch_bytes(int B, int N, int H8, int W8);
int    pips_mixer_input_build_tiled(const float* pyramid, int B, int S, int H8, int W8,
                                    const float* ffeats, const float* coords, const float* times,
                                    int N, float* X, void* scratch, size_t scratch_bytes, void* stream);
int    pips_mixer_input_build_tiled_timed(const float* pyramid, int B, int S, int H8, int W8,
                                          const float* ffeats, const float* coords, const float* times,
                                          int N, float* X, void* scratch, size_t scratch_bytes, void* stream,
                                          float* ms3_host);
/* The same with flags.  PIPS_FLAG_BF16_MAPS: the bf16 mode of a dense query set -- under torch.autocast the reference correlates
 * bf16 features with bf16 maps (nets/pips.py:394-397), so the work items of the tiled path run on the matrix cores
 * (gather_mfma_kernel: the tile's region of the pyramid's bf16 MIRROR times all of the item's particles' features, rounded to
 * bf16, as v_mfma_f32_32x32x16_bf16 products with fp32 sums; each particle keeps its 8 x 8 window; same blend, same taps).
 * pips_forward / pips_track take this route by themselves when PIPS_FLAG_BF16_MAPS is set and the query set is dense.
 * ms3_host != NULL: as the _timed form ({bin_particles, embed_rows, gather} ms; synchronises the stream). */
/* Which correlation-gather kernel pips_forward / pips_track (8 frames per clip, no per-particle windows) run for this query set:
 * 0 = the direct kernel (mixer_input_kernel, or mixer_input_bf16maps_kernel with PIPS_FLAG_BF16_MAPS), 1 = gather_tiled_kernel
 * (fp32, LDS-tiled), 2 = gather_mfma_kernel (PIPS_FLAG_BF16_MAPS on a dense query set).  Host function; needs a current device. */
int    pips_gather_route(int B, int N, int H8, int W8, int flags);
int    pips_mixer_input_build_tiled_ex(const float* pyramid, int B, int S, int H8, int W8,
                                       const float* ffeats, const float* coords, const float* times,
                                       int N, int flags, float* X, void* scratch, size_t scratch_bytes,
                                       void* stream, float* ms3_host);

/* MLPMixer (nets/pips.py:111-123): X (M,544) -> delta (M/8, 1040).  M = B*N*8. */
size_t pips_mixer_workspace_bytes(int M);
int    pips_mixer_fwd(const void* arena, const float* X, int M, float* delta,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Same with bf16 MFMA operands (PIPS_FLAG_BF16_MIXER): weights converted once at pack time,
 * activations rounded to bf16 (RNE) as they are staged, fp32 accumulation and epilogues. */
int    pips_mixer_fwd_bf16(const void* arena, const float* X, int M, float* delta,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Same with every GEMM on the split-bf16 (bf16x3) path: fp32-grade results, see pips_gemm_f32x3. */
int    pips_mixer_fwd_x3(const void* arena, const float* X, int M, float* delta,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Profiling variant (the ONLY entry point that creates events and synchronises): same work as
 * pips_mixer_fwd with a hipEvent pair around every GEMM launch on `stream`; ms_host[5] receives
 * {in-proj, mean of the 12 up-projections (512->2048 +GELU), mean of the 12 down-projections
 * (2048->512 +residual), head, marker-pair overhead (empty event pair)} in milliseconds, the
 * first four RAW (not overhead-corrected).  Used by bench.py for the roofline object. */
int    pips_mixer_fwd_timed(const void* arena, const float* X, int M, float* delta,
                            void* workspace, size_t workspace_bytes, void* stream, float* ms_host);
/* Same for the matrix mode selected by flags (0, PIPS_FLAG_BF16_MIXER or PIPS_FLAG_SPLIT_BF16). */
int    pips_mixer_fwd_timed_ex(const void* arena, const float* X, int M, int flags, float* delta,
                               void* workspace, size_t workspace_bytes, void* stream, float* ms_host);

/* Profiling: the two channel-mix Linear shapes (nets/pips.py:102-109) as launch trains -- the 12 layers' up-projections, then
 * their down-projections, back to back on the layers' own weights between ONE HIP event pair, `reps` times.
 * ms2_host = {up-projection, down-projection} milliseconds PER LAUNCH, start to start as the forward pays them (no per-launch
 * marker, nothing subtracted).  The workspace must hold a mixer pass at this M (pips_mixer_fwd* on it first).  bench.py's
 * roofline.frac comes from this. */
int    pips_mixer_gemm_train(const void* arena, int M, int flags, void* workspace, size_t workspace_bytes,
                             void* stream, int reps, float* ms2_host);

/* State update nets/pips.py:525-539 (+ vis head :559 when out_vis != NULL).
 * delta (B*N,1040); ffeats/coords updated in place; coords0 = locked frame-0 coords;
 * out_traj (B,S,N,2) receives coords*stride. */
int    pips_state_update(const void* arena, const float* delta, float* ffeats, float* coords,
                         const float* coords0, int B, int N, float stride,
                         float* out_traj, float* out_vis, void* stream);
/* The same for an arena packed at any window length S in 1 .. PIPS_S_MAX (PIPS_E_ARG otherwise): delta rows are
 * pips_delta_stride(S) floats apart, ffeats (B*N,S,128), coords / coords0 (B*N,S,2), out_traj (B,S,N,2), out_vis (B,S,N) or NULL.
 * pips_state_update is its S = 8 form (same kernel, same bits). */
int    pips_state_update_s(const void* arena, const float* delta, float* ffeats, float* coords,
                           const float* coords0, int B, int N, int S, float stride,
                           float* out_traj, float* out_vis, void* stream);

/* The mixer's and the update's stage kernels, one launch each (exposed for unit tests; additive, the ABI version stays).  Every
 * one answers PIPS_E_ARG ahead of any launch for a NULL pointer it would use, a size below 1, S outside 1 .. PIPS_S_MAX and the
 * cases named; none does arithmetic of its own -- each is the launch pips_mixer_fwd_s / pips_track_s make, on the offsets of an
 * arena packed for S.
 *
 * flags (pips_token_mix, pips_ln_mean): 0, PIPS_FLAG_BF16_MIXER, or PIPS_FLAG_BF16_MIXER | PIPS_FLAG_BF16_STREAM (S = 8 only);
 * anything else is PIPS_E_ARG.
 *
 * pips_token_mix: the token-mixing half of mixer layer `layer` (0 .. 11; nets/pips.py:93-109) and the LayerNorm in front of the
 * channel mixing: x [particles][S][512] += TokenMLP(LN1(x)) in place (fp32, or bf16 with BF16_STREAM), xn = LN2(new x), fp32 or
 * (both bf16 modes) bf16.
 * pips_ln_mean: the final LayerNorm and the mean over the S tokens (:120-121): out [particles][512] fp32; x as above.
 * pips_vis_head: vis_predictor (:421-426) on ffeats (B*N,S,128): out_vis (B,S,N). */
int    pips_token_mix(const void* arena, int layer, void* x, void* xn, int particles, int S, int flags, void* stream);
int    pips_ln_mean(const void* arena, const void* x, float* out, int particles, int S, int flags, void* stream);
int    pips_vis_head(const void* arena, const float* ffeats, int B, int N, int S, float* out_vis, void* stream);

/* Generic fp32-MFMA building blocks (exposed for unit tests).
 * C[M,N] = epi(A[M,K] * W[N,K]^T + bias[N]); K % 32 == 0; epi: 0 none, 1 GELU(erf),
 * 2 add residual R (ldr). */
int    pips_gemm_f32(const float* A, int lda, const float* W, const float* bias,
                     float* C, int ldc, int M, int N, int K, int epi,
                     const float* R, int ldr, void* stream);
/* NHWC convolution as implicit GEMM, weights [Cout][kh][kw][Cin], Cin % 32 == 0.
 * stats (optional) receives InstanceNorm partials of the output about a pivot, float4 {sum(x-p), sum((x-p)^2), p, n}
 * per (frame, part, channel), part = m-tile x wave row: room for F * (2*ceil(Ho*Wo/64) + 4) * Cout * 4 floats;
 * returns the number of parts per frame through *tiles_m_host. */
int    pips_conv_nhwc_f32(const float* in, int F, int H, int W, int Cin,
                          const float* wgt, const float* bias, int Cout, int ksize, int cstride, int pad,
                          float* out, float* stats, int* tiles_m_host, void* stream);
/* pips_conv_nhwc_f32 on a named kernel (exposed for unit tests): PIPS_CONV_ROUTE_AUTO = the kernel the shape selects (what
 * pips_conv_nhwc_f32 runs), PIPS_CONV_ROUTE_IGEMM = igemm_f32_kernel, PIPS_CONV_ROUTE_E = the 64 x 64 LDS-DMA body (1x1 or 3x3,
 * stride 1 or 2, pad = ksize / 2, Cin 64 / 96 / 128 and, 1x1 only, 256, bias required; PIPS_E_ARG otherwise).  Both named kernels
 * write 2*ceil(Ho*Wo/64) parts per frame on 64-row tiles. */
#define PIPS_CONV_ROUTE_AUTO   0
#define PIPS_CONV_ROUTE_IGEMM  1
#define PIPS_CONV_ROUTE_E      2
#define PIPS_CONV_ROUTE_R      3      /* the LDS-resident 64 -> 64 kernel: through pips_conv_nhwc_f32_r only */
int    pips_conv_nhwc_f32_route(const float* in, int F, int H, int W, int Cin,
                                const float* wgt, const float* bias, int Cout, int ksize, int cstride, int pad,
                                float* out, float* stats, int* tiles_m_host, int route, void* stream);
/* The LDS-resident 3x3 convolution of the fp32 encoder's layer 1 (conv3x3_c64_f32_r_kernel; exposed for unit tests) at ANY map
 * size, whatever pips_encoder_l1_fused says: weights of all nine taps and the input patch of a 4 x 32 pixel tile in LDS, exact fp32
 * products in the K order of PIPS_CONV_ROUTE_IGEMM -- the output map is bitwise that route's.  in_norm (optional): {mean, rstd} per
 * (frame, input channel) of the layer that produced `in`; fmaxf((x - mean) * rstd, 0) -- bitwise pips_inorm_apply's mode 0 -- is
 * applied to the map while it is staged, taps outside the image stay zero.  stats (required) receives 4*ceil(H/4)*ceil(W/32) parts
 * per frame (returned through *parts_host): one per image row of every tile, n = 0 for the rows below the image;
 * stats_parts_cap = room in stats in parts per frame (0 = the 2*ceil(H*W/64)+4 of pips_conv_nhwc_f32).  PIPS_E_ARG: anything but
 * ksize 3, cstride 1, pad 1, Cin = Cout = 64, a bias, stats, parts within the cap and a map of (H+2)*(W+2)*256 < 2^31 bytes. */
int    pips_conv_nhwc_f32_r(const float* in, const float* in_norm, int F, int H, int W, int Cin,
                            const float* wgt, const float* bias, int Cout, int ksize, int cstride, int pad,
                            float* out, float* stats, int stats_parts_cap, int* parts_host, void* stream);
/* 1 if pips_encoder_fwd (exact fp32) runs layer 1 of F frames of H x W pixels on that kernel -- its four convolutions normalise
 * their input while staging it, so three normalised half-resolution maps are never stored -- 0 if it runs the staged sequence
 * (fewer than a threshold of tiles per compute unit).  Host function; needs a current device. */
int    pips_encoder_l1_fused(int F, int H, int W);

/* The finalize of those partials (exposed for unit tests): partial (F, parts, C) float4 -> mean_rstd (F, C, 2) = {mean,
 * 1 / sqrt(var + 1e-5)}, combined in fp64; C % 16 == 0. */
int    pips_inorm_finalize_pivot(const float* partial, int F, int parts, int C, float* mean_rstd, void* stream);

/* The encoder's kernels that are not convolutions of a map, one launch each (exposed for unit tests; additive, the ABI version
 * stays).  Every one answers PIPS_E_ARG ahead of any launch for a NULL pointer it would use, a size below 1 and the cases named.
 *
 * pips_encoder_stem: conv1 of BasicEncoder (7x7, stride 2, pad 3, 3 -> 64; nets/pips.py:251) with the 2*(x/255)-1 of :436 on the
 * caller's (F,3,H,W) frames, on the weights of a packed arena.  flags = 0 | PIPS_FLAG_BF16_ENCODER | PIPS_FLAG_RGB_U8 (anything else:
 * PIPS_E_ARG): rgbs float or uint8; out = the RAW map [F][Ho][Wo][64], Ho = (H - 1) / 2 + 1, fp32 or (bf16 mode) bf16; stats =
 * pivoted InstanceNorm partials float4 {sum(x-p), sum((x-p)^2), p, n} [F][parts][64] taken from the fp32 accumulators, parts =
 * pips_encoder_stem_parts(H, W) (0 for a size below 1), also returned through *parts_host (may be NULL). */
int    pips_encoder_stem_parts(int H, int W);
int    pips_encoder_stem(const void* arena, const void* rgbs, int F, int H, int W, int flags, void* out, float* stats,
                         int* parts_host, void* stream);
/* InstanceNorm apply + ReLU + shortcut on NHWC maps [F][HW][C], fp32 (maps_bf16 = 0, C % 4 == 0) or bf16 (C % 8 == 0, C <= 2048),
 * with n(x) = (x - mean) * rstd from stats (F, C, 2):  mode 0: y = relu(n(x));  1: relu(res + relu(n(x)));  2: relu(n2(res) +
 * relu(n(x))), n2 from res_stats;  3 (bf16 maps only): relu(relu(n2(res)) + relu(n(x))).  PIPS_E_ARG: a mode outside 0..2 (0..3
 * with bf16 maps), a mode >= 1 without res, a mode >= 2 without res_stats, a C off its alignment. */
int    pips_inorm_apply(const void* x, const float* stats, const void* res, const float* res_stats, int mode, void* y,
                        int F, int HW, int C, int maps_bf16, void* stream);
/* pips_inorm_apply on fp32 maps with every mode of the bf16 form: modes 0..2 as above (the same kernels), and mode 3,
 * relu(relu(n2(res)) + relu(n(x))) -- a residual block's closing pass when the block's input exists only as the RAW map of the layer
 * that produced it (the fused layer 1 of the fp32 encoder, pips_encoder_l1_fused): the same fp32 operations in the same order as mode 0
 * on each operand followed by relu(a + b).  PIPS_E_ARG: a mode outside 0..3, a mode >= 1 without res, a mode >= 2 without res_stats,
 * C % 4 != 0 or C > 2048. */
int    pips_inorm_apply_f32(const float* x, const float* stats, const float* res, const float* res_stats, int mode, float* y,
                            int F, int HW, int C, void* stream);
/* F.interpolate(mode='bilinear', align_corners=True) (nets/pips.py:269-272) of an NHWC map [F][Hs][Ws][C] into channels
 * [coff, coff + C) of the NHWC map dst [F][Hd][Wd][Cdst] (the torch.cat of :273); the other channels of dst are not written.
 * fp32 maps (C, Cdst, coff multiples of 4) or bf16 maps (multiples of 8).  PIPS_E_ARG: coff < 0, coff + C > Cdst, alignment. */
int    pips_resize_into(const void* src, int F, int Hs, int Ws, int C, void* dst, int Hd, int Wd, int Cdst, int coff,
                        int maps_bf16, void* stream);
/* F.avg_pool2d(x, 2, stride=2) (nets/pips.py:349) of an fp32 NHWC map [F][H][W][C] -> [F][H/2][W/2][C]; C % 4 == 0, H, W >= 2. */
int    pips_avgpool2(const float* src, int F, int H, int W, int C, float* dst, void* stream);

/* epi values of the GEMM building blocks; PIPS_EPI_RES_BF16 is OR-ed to PIPS_EPI_RESIDUAL for pips_gemm_bf16 with out_bf16 = 1:
 * the residual R is a bf16 tensor too (the mixer's bf16 residual stream, PIPS_FLAG_BF16_STREAM).  Any other combination with it is
 * rejected (PIPS_E_ARG) -- without out_bf16 a bf16 R would be read as fp32. */
#define PIPS_EPI_BIAS      0
#define PIPS_EPI_GELU      1
#define PIPS_EPI_RESIDUAL  2
#define PIPS_EPI_RES_BF16  0x1000
/* bf16-operand building block (BASELINE config 3): A fp32 (rounded to bf16 while staged) or bf16 [M][lda], W bf16 [N][K]
 * (round-to-nearest-even of the fp32 weights), fp32 accumulation, C fp32 or bf16 [M][ldc]; epi as pips_gemm_f32
 * (+ PIPS_EPI_RES_BF16).  K % 32 == 0 (K % 64 unless A and C are fp32). */
int    pips_gemm_bf16(const void* A, int a_bf16, int lda, const void* W, const float* bias, void* C, int out_bf16, int ldc,
                      int M, int N, int K, int epi, const float* R, int ldr, void* stream);
/* Which kernel pips_gemm_bf16 (and the bf16 mixer of pips_forward) takes for a problem with bias and, for epi = residual, an
 * fp32 residual of ldr = N: 0 = register-staged gemm_bf16_kernel; 3 = gemm_bf16_t4_res_kernel (down-projection: bf16 A, fp32 C,
 * bias + residual, M % 128 == 0, N % 256 == 0, K % 64 == 0, at least half a 128 x 256 tile per compute unit); 4 =
 * gemm_bf16_t4_gelu_kernel (up-projection: bf16 A and C, GELU, K = 512, M and N multiples of 256, at least three quarters of a 256 x 256
 * tile per compute unit; rounds the Linear output to bf16 ahead of the GELU as autocast does).  Both are four-wave kernels on
 * v_mfma_f32_16x16x32_bf16 with a generated static schedule (1 and 2 were kernels of rounds 2-3).  Host function;
 * needs a current device.  The mixer's bf16 numerics depend on M = B*N*8 through this choice. */
int    pips_gemm_bf16_route(int M, int N, int K, int epi, int a_bf16, int out_bf16);

/* Which kernel pips_gemm_f32 (and the fp32 mixer of pips_forward) takes for a problem with bias and, for epi = residual, a residual of
 * ldr = N: 0 = igemm_f32_kernel (gemm.hip); 1 = gemm_f32_t4u_kernel (128 x 128 tiles: epi GELU or residual, M and N multiples of
 * 128, K % 64 == 0, at least three quarters of a tile per compute unit); 2 = gemm_f32_t4e_kernel (64 x 64 tiles, LDS-DMA staging; the K range split
 * over the four waves and summed in a fixed order: epi residual, K % 128 == 0, between 0.75 and 2 tiles per compute unit -- the
 * down-projection at M = 2048).  Same exact-fp32 MFMA arithmetic everywhere; 1 is bitwise igemm_f32_kernel's unsplit form, 2
 * differs from it by the order of the four partial sums.  Host function; needs a current device. */
int    pips_gemm_f32_route(int M, int N, int K, int epi);
/* Compute units of the current device (0: no device).  Every "tiles per compute unit" threshold of the route functions is
 * relative to this number; tests derive their route expectations from it instead of assuming 256. */
int    pips_device_cus(void);

/* pips_conv_nhwc_f32 with bf16 MFMA operands: the fp32 map is rounded to bf16 while it is staged, wgt_bf16 is the
 * round-to-nearest-even bf16 copy of the [Cout][kh][kw][Cin] weights; fp32 accumulation and output, same stats. */
int    pips_conv_nhwc_bf16(const float* in, int F, int H, int W, int Cin,
                           const void* wgt_bf16, const float* bias, int Cout, int ksize, int cstride, int pad,
                           float* out, float* stats, int* tiles_m_host, void* stream);

/* The same convolution on bf16 MAPS (what the bf16 encoder mode uses between its layers): in_bf16 is a bf16 NHWC map;
 * in_norm (optional, 64 -> 64 3x3 stride-1 layers on maps the LDS-resident kernel takes: >= 512 tiles of 4x64 pixels)
 * holds {mean, rstd} per (frame, input channel) of the layer that produced the map, and relu((x - mean) * rstd) is
 * applied to it while it is staged (taps outside the image stay zero); out is bf16 (out_is_bf16) or fp32; the
 * statistics are taken from the fp32 accumulators.  stats_parts_cap = room in stats in partials per frame (0 = the
 * 2*ceil(Ho*Wo/64)+4 of pips_conv_nhwc_f32); the ping-pong 64 -> 64 kernel wants ceil(W/32)*ceil(H/4)*4 and is
 * only taken when that fits. */
int    pips_conv_nhwc_bf16_maps(const void* in_bf16, const float* in_norm, int F, int H, int W, int Cin,
                                const void* wgt_bf16, const float* bias, int Cout, int ksize, int cstride, int pad,
                                void* out, int out_is_bf16, float* stats, int stats_parts_cap, int* tiles_m_host,
                                void* stream);

/* Split-bf16 ("bf16x3") building blocks: fp32-grade results from the bf16 matrix cores.  Every
 * fp32 operand is split exactly into three bf16 terms and each product is formed from six exact
 * bf16 products accumulated in fp32 (same F.linear / F.conv2d contracts as the two calls above).
 * pips_split_bf16x3: src fp32 [n] (n even) -> dst bf16 planes [3][n] (6n bytes).
 * pips_gemm_f32x3 / pips_conv_nhwc_f32x3: W3 / wgt3 are the split planes of the fp32 weights. */
int    pips_split_bf16x3(const float* src, size_t n, void* dst3, void* stream);
int    pips_gemm_f32x3(const float* A, int lda, const void* W3, const float* bias,
                       float* C, int ldc, int M, int N, int K, int epi,
                       const float* R, int ldr, void* stream);
int    pips_conv_nhwc_f32x3(const float* in, int F, int H, int W, int Cin,
                            const void* wgt3, const float* bias, int Cout, int ksize, int cstride, int pad,
                            float* out, float* stats, int* tiles_m_host, void* stream);

/* Score-map loss terms of nets/pips.py:501-511 + score_map_loss :58-92 (evaluation: test_on_flt.py:87 and
 * test_on_crohd.py:133 pass trajs_g / vis_g / valids).  pips_forward_ce / pips_track_ce are pips_forward / pips_track
 * plus: ce_tgt (B*N*S,3) = per mixer row m=(b*N+n)*S+s {x, y, use}: the rounded target pixel in map coordinates
 * (trajs_g/stride rounded half-to-even) and use = 1 when that heat map enters the loss (target inside the map,
 * valids > 0, vis_g > 0), else 0;  ce_terms (iters, B*N*S, 2) receives per iteration and row {loss at the target
 * pixel, sum of the losses of all other pixels} (balanced_ce_loss's stable softplus, :26-29) -- the caller divides
 * the two totals by (#used rows * iters) and (#used rows * iters * (H8*W8 - 1)) (+1e-6, utils.basic.reduce_masked_mean)
 * and adds them;  ce_ws: pips_score_map_workspace_bytes(B,S,H8,W8) of scratch (the four pyramid levels upsampled and
 * summed once: the (B,S,N,H8,W8) volume itself is never formed).  ce_tgt == NULL: exactly pips_forward / pips_track.
 * pips_score_map_prepare / _terms are the two stages on their own (_terms on any U of B*S frames of H8 x W8 pixels; PIPS_E_ARG
 * ahead of the launch for a NULL pointer or B, S, N, H8 or W8 below 1). */
size_t pips_score_map_workspace_bytes(int B, int S, int H8, int W8);
int    pips_score_map_prepare(const float* pyramid, int B, int S, int H8, int W8, float* U, void* stream);
int    pips_score_map_terms(const float* U, int B, int S, int H8, int W8, const float* ffeats, int N,
                            const float* tgt, float* out, void* stream);
int    pips_forward_ce(const void* arena, const float* rgbs, const float* xys,
                       const float* coords_init, const float* feat_init, const float* times,
                       int B, int S, int H, int W, int N, int stride, int iters, int flags,
                       void* workspace, size_t workspace_bytes,
                       float* out_trajs, float* out_vis, float* out_ffeat0,
                       const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes, void* stream);
int    pips_track_ce(const void* arena, const float* pyramid, int B, int T, int H8, int W8,
                     const float* xys, const float* coords_init, const float* feat_init,
                     const int* win_start, const float* times, int N, int stride, int iters, int flags,
                     void* workspace, size_t workspace_bytes,
                     float* out_trajs, float* out_vis, float* out_ffeat0,
                     const float* ce_tgt, float* ce_terms, void* ce_ws, size_t ce_ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIPS_HIP_H */
