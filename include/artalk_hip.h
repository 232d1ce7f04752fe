/* C ABI of libartalk_hip.so: the MI355X (gfx950) implementation of ARTalk's audio->motion path.
 *
 * The reference has no FFI layer; its operator boundary is the Python object stored in
 * ARTAvatarInferEngine.ARTalk (reference inference.py:27).  The entry points below are what a binding
 * for that object needs, one per call the reference makes across the boundary:
 *
 *   artalk_create            <- BitwiseARModel(configs).eval().to(device)        inference.py:27, app/models.py:14-56
 *   artalk_set_tensor        <- one state_dict entry of load_state_dict(strict)  inference.py:28
 *   artalk_finalize_weights  <- end of load_state_dict(strict=True): missing keys are an error
 *   artalk_infer             <- BitwiseARModel.inference(batch)                  inference.py:50, app/models.py:62-121
 *                               (batched: B independent batch-1 runs; the reference asserts B==1, app/models.py:65)
 *   artalk_savgol            <- ARTAvatarInferEngine.smooth_motion_savgol        inference.py:89-95
 *   artalk_destroy           <- object lifetime
 *   artalk_pcm_*             <- torchaudio.load + Resample(sr, 16000)(x).mean(0)  inference.py:230-231, for a live sender: raw PCM
 *                               packets in, the model's 16 kHz blocks out, the bits of the whole-clip call ("Live audio in" below)
 *
 * Conventions: plain pointers and sizes only; all *_dev pointers are device memory on the model's GPU;
 * every call returns 0 on success or a negative ARTALK_E* code (text via artalk_last_error); the caller
 * owns every buffer it passes; the library owns weights and workspace; one model per GPU, calls on one
 * model are not thread-safe; work is enqueued on the hipStream_t passed as `stream` (NULL = a stream the
 * library owns) and artalk_infer / artalk_stream_* return without synchronising: the small host tables of a
 * call (chunk offsets, style flags) go through a ring of pinned staging slots, so a call blocks only when
 * four earlier calls are still in flight, or when it has to grow the workspace (artalk_reserve avoids that).
 *
 * The artalk_op_* entry points expose single kernels so that tests can check each one against the CPU
 * oracle through this same ABI; they are not needed by a binding.
 */
#ifndef ARTALK_HIP_H
#define ARTALK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARTALK_OK 0
#define ARTALK_EINVAL (-1)      /* bad argument / shape mismatch                      */
#define ARTALK_EKEY (-2)        /* unknown state_dict key (strict=True)               */
#define ARTALK_EMISSING (-3)    /* finalize with keys missing (strict=True)           */
#define ARTALK_EHIP (-4)        /* HIP runtime error                                  */
#define ARTALK_ESTATE (-5)      /* call order (infer before finalize, ...)            */
#define ARTALK_ECAPACITY (-6)   /* batch larger than the reserved workspace           */
#define ARTALK_EBUSY (-7)       /* artalk_poll_status: the call is still running      */

#define ARTALK_DTYPE_F32 0
#define ARTALK_DTYPE_I64 1

typedef struct artalk_model artalk_model;

/* assets/config.json + the XLS-R-300M hyper-parameters (reference app/models.py:25) */
typedef struct artalk_config {
    int32_t ar_depth, ar_heads;                 /* AR_CONFIG.T_DEPTH, T_NUM_HEADS (PREV_RATIO must be 1)  */
    int32_t vae_depth, vae_heads, vae_hidden;   /* VAE_CONFIG.T_DEPTH, T_NUM_HEADS, T_HIDDEN_DIM          */
    int32_t code_dim, motion_dim;               /* 32, 106                                                */
    int32_t n_levels; int32_t patch_nums[8];    /* 5; 1,5,25,50,100                                       */
    int32_t w2v_layers, w2v_hidden, w2v_heads, w2v_ffn;
    int32_t w2v_n_conv; int32_t w2v_conv_kernel[8]; int32_t w2v_conv_stride[8]; int32_t w2v_conv_dim;
    int32_t w2v_pos_kernel, w2v_pos_groups;
    float w2v_ln_eps;
    int32_t style_dim, style_heads, style_layers, style_ffn, style_len;
} artalk_config;

int artalk_create(int device_id, const artalk_config* cfg, artalk_model** out);
void artalk_destroy(artalk_model* m);
const char* artalk_last_error(const artalk_model* m);   /* m may be NULL: error of the last failed create */

/* One call per state_dict entry, host memory, reference key names. */
int artalk_set_tensor(artalk_model* m, const char* key, const void* host_ptr, int dtype, int ndim, const int64_t* shape);
/* Folds weight-norm, re-lays out conv weights, builds fused tables.  ARTALK_EMISSING lists missing keys in last_error. */
int artalk_finalize_weights(artalk_model* m);

/* Allocate workspace for up to max_batch clips and max_total_chunks 4-second chunks per artalk_infer call. */
int artalk_reserve(artalk_model* m, int max_batch, int max_total_chunks);
int64_t artalk_workspace_bytes(const artalk_model* m);
int64_t artalk_weight_bytes(const artalk_model* m);

/* Audio -> FLAME codes for B independent clips.
 *   audio_dev        [B][audio_clip_stride] f32, 16 kHz mono; clip b holds n_chunks[b]*64000 samples, zero padded
 *                    by the caller exactly as app/models.py:78-85 pads.
 *   n_chunks         host, [B], must be non-increasing (the host sorts clips; ragged batches stay dense prefixes).
 *   style_motion_dev [B][50][106] f32 or NULL; has_style host [B] (NULL = none): app/models.py:67-73.  has_style[b] = 1: row b
 *                    is a style clip; 2: the first 768 floats of row b are a condition computed by artalk_style_encode
 *                    (the style-clip cache: the encoder is skipped); 0: no style (null_style_cond).
 *   out_motion_dev   [B][out_clip_stride] f32, receives n_chunks[b]*100 rows of 106 per clip (caller truncates
 *                    to ceil(N/640) rows, app/models.py:115).
 *   out_bits_dev     optional [B][max_chunks][181][32] u8: the 0/1 decisions of app/models.py:104 (last scale step).
 *   out_hist_bits_dev optional [B][max_chunks+1][181][32] u8: history bits of bitwise_vae.py:78-93 (index 0 = initial).
 *   out_w2v_dev      optional [total_chunks][199][1024] f32 wav2vec2 features, chunk order (chunk index major, clip minor).
 */
int artalk_infer(artalk_model* m, const float* audio_dev, int64_t audio_clip_stride, const int64_t* n_chunks, int B,
                 const float* style_motion_dev, const uint8_t* has_style, float* out_motion_dev, int64_t out_clip_stride,
                 uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, float* out_w2v_dev, void* stream);

/* artalk_infer for clips whose length the caller knows: n_samples host, [B], the real samples of clip b (1 .. n_chunks[b]*64000); what
 * follows them up to n_chunks[b] whole chunks MUST be zeros.  The wav2vec2 conv stack has no padding and mixes no frames, so every
 * frame of a chunk that hears the zero padding alone equals the first such frame bit for bit: the stack computes that one and copies
 * it (chunks in length classes by quarter of a chunk, one pass per class).  Same results as artalk_infer, bit for bit, in every
 * precision mode; n_samples = NULL is artalk_infer (every chunk runs whole).  artalk_set_tail_skip(m, 0) runs every chunk whole
 * whatever the counts say (default 1): the A/B and test switch.  The streaming calls always run whole chunks. */
int artalk_infer_samples(artalk_model* m, const float* audio_dev, int64_t audio_clip_stride, const int64_t* n_chunks,
                         const int64_t* n_samples, int B, const float* style_motion_dev, const uint8_t* has_style, float* out_motion_dev,
                         int64_t out_clip_stride, uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, float* out_w2v_dev, void* stream);
int artalk_set_tail_skip(artalk_model* m, int on);
/* The geometry behind it (host only, no device): for a chunk of samples_per_chunk samples with `valid` (1 .. samples_per_chunk) real ones
 * and the conv table kernel[n_conv] / stride[n_conv] (stride 2 from layer 1 on), per layer i: t_const[i], the first output row whose
 * receptive field starts at or after sample `valid`; Tp[i], the rows to compute - the last layer's rows up to and including
 * t_const[last], counted back as Tp[i-1] = (Tp[i] - 1) stride[i] + kernel[i]; Sp[i], the per-chunk row stride (Sp[last] = Tp[last] + 1,
 * Sp[i-1] = 2 Sp[i] >= Tp[i-1]); *samples_read, the samples layer 0 then reads.  Returns 1, or 0 when t_const[last] is the last row
 * or beyond (nothing to skip: Tp / Sp are the whole chunk's), or ARTALK_EINVAL.  artalk_conv_tail_class: the upper bound, in
 * samples, of the length class (quarters of a chunk) a chunk with `valid` real samples runs at. */
int artalk_conv_tail_geometry(int64_t valid, int samples_per_chunk, int n_conv, const int* kernel, const int* stride, int* t_const,
                              int* Tp, int* Sp, int* samples_read);
int64_t artalk_conv_tail_class(int64_t valid, int samples_per_chunk);

/* Style condition of n style clips (app/models.py:67-73: StyleEncoder -> style_cond_embed -> 1.1 c - 0.1 null), for callers that
 * keep one style across many calls as the reference's engine does (inference.py:41-45): style_motion_dev [n][50][106] ->
 * out_cond_dev [n][768].  Pass a condition back through artalk_infer / artalk_stream_begin with has_style[b] = 2. */
int artalk_style_encode(artalk_model* m, const float* style_motion_dev, int n, float* out_cond_dev, void* stream);

/* Streaming form of the same path (chunk-at-a-time, history kept in the model between calls): the reference
 * loop body of app/models.py:92-114 for B parallel streams.  artalk_stream_begin computes the style condition and the initial
 * history (app/models.py:67-73,86-89); every artalk_stream_chunk consumes the next 64000 samples of each stream
 * (audio_dev [B][chunk_stride], zero padded by the caller at the end of a clip) and writes 100 x 106 codes per stream to
 * out_motion_dev [B][out_stride].  artalk_stream_end, a new artalk_stream_begin or a call to artalk_infer ends the session
 * (shared workspace); growing the workspace (artalk_reserve) ends it too, and artalk_stream_chunk then fails with ARTALK_ESTATE. */
int artalk_stream_end(artalk_model* m);
int artalk_stream_begin(artalk_model* m, int B, const float* style_motion_dev, const uint8_t* has_style, void* stream);
int artalk_stream_chunk(artalk_model* m, const float* audio_dev, int64_t chunk_stride, float* out_motion_dev, int64_t out_stride,
                        void* stream);

/* Independent streaming sessions: the same chunk step for streams that join and leave between steps (a server with live users).
 * What a stream carries from chunk to chunk - style condition [768], history tokens [181][768], decoder features of the previous
 * chunk [100][32], fp32 in every precision mode: 571 904 bytes, and behind them the streaming smoother's carry, the last 9 raw frames
 * [9][106] padded to 16 bytes: 3 824 bytes - lives in a session pool owned by the model, outside the workspace:
 * device blocks of 32 slots that are never moved or freed before artalk_destroy.  A step gathers the listed sessions into workspace
 * rows 0..n-1 (one copy kernel), runs there what artalk_stream_chunk runs for n streams - the same rows, hence the same captured
 * graphs and the same bits - and scatters the new history back (one copy kernel); nothing synchronises.  Between library calls the
 * workspace holds nothing a session needs.
 *   Lifetime: sessions survive artalk_infer, artalk_style_encode, artalk_stream_begin / _chunk / _end and workspace growth
 * (artalk_reserve, a larger call); artalk_set_precision (the state is fp32 and every mode reads it the same way; a session may change
 * mode between steps); artalk_set_graphs, artalk_set_cu_mask, the audit, tap and profiling switches (while one of them forbids
 * graphs, a step runs eagerly, by the rule of every other call).  A change of site scales - artalk_calibrate, artalk_set_site_scales
 * or artalk_reset_scales that changed an exponent - closes ALL sessions (a session never mixes exponents): the next artalk_session_step
 * with such an id fails with ARTALK_ESTATE and a message that says so.  In the other direction artalk_session_open and
 * artalk_session_step end a lockstep session (artalk_stream_begin), as artalk_infer does: they rewrite the workspace rows it lives in.
 * Calls for one model are ordered by the caller, as for artalk_infer (a step reads what the previous step of the same session wrote).
 *
 * artalk_sessions_reserve  allocates pool blocks for at least max_sessions sessions (optional: artalk_session_open grows the pool on
 *                          demand, one hipMalloc per 32 sessions).
 * artalk_session_open      opens n sessions: style arguments and validation of artalk_stream_begin (style_motion_dev [n][50][106] or
 *                          NULL, has_style host [n] with flags 0, 1, 2); computes style condition and initial history in the workspace and
 *                          stores them in n free slots.  ids_out host [n] receives the ids: positive, never reused during the model's
 *                          life (a freed slot is reused under a new id).  Publishes a status word (a ticket) like artalk_stream_begin.
 * artalk_session_step      the next 64000 samples of the n listed sessions, any subset of the open ones in any order: row i of audio_dev
 *                          [n][chunk_stride] and of every output belongs to ids[i].  out_motion_dev [n][out_stride] receives 100 x 106
 *                          codes per session; out_bits_dev (optional) [n][181][32] u8 this chunk's AR decisions, out_hist_bits_dev
 *                          (optional) [n][181][32] u8 the bits of the new history.  The status word is reset at the start of every step
 *                          and published at its end: each step has its own ticket.  The workspace grows when n exceeds it.  ARTALK_EINVAL
 *                          for n <= 0, an id that is not open (never issued, closed) or listed twice: nothing is enqueued, no session
 *                          changes.  The caller zero-pads the last chunk of a clip, as for artalk_stream_chunk.
 * artalk_session_close     frees the slots of the n listed sessions (host bookkeeping only; ordered by the caller against the steps
 *                          that still use them).  ARTALK_EINVAL, with nothing changed, for an id that is not open or listed twice; an id
 *                          that a scale change closed is accepted.
 * artalk_session_count     number of open sessions.
 * artalk_session_smooth    smooth_motion_savgol (inference.py:89-95: savgol_filter (5, 2) on every dim, (9, 3) on dims 100:103, mode='interp')
 *                          for live sessions: bit for bit what artalk_savgol gives on the session's concatenated codes, 4 frames (160 ms)
 *                          late - the filter's half width.  Row i of raw_dev [n][raw_stride] holds the n_frames[i] codes (0..100) the last
 *                          artalk_session_step produced for ids[i]; last[i] says that the stream ends with them.  n_frames, last: host [n]
 *                          (NULL: 100 / 0 everywhere).  With T' = frames consumed so far + n_frames[i], row i of out_dev [n][out_stride]
 *                          (out_stride >= 104 x 106) receives the stream frames [max(0, T' - n_frames[i] - 4), T' - 4), or up to T' with
 *                          last[i]; first_out / count_out (host [n], filled before the call returns) say which: 96 frames on a stream's
 *                          first call, 100 afterwards, up to 104 at the end.  Rows of out_dev at index count_out[i] and beyond are left
 *                          untouched, rows of raw_dev at index n_frames[i] and beyond are not read.  n_frames[i] == 0 with last[i] is the
 *                          flush of a stream that ended on a chunk boundary: the pending 4 frames, raw_dev row i (or a NULL raw_dev) is not
 *                          read.  Checked before anything is enqueued or any session changes: ARTALK_EINVAL for an id that is not open or
 *                          listed twice (ARTALK_ESTATE, with artalk_session_step's message, for one a scale change closed), for n_frames
 *                          outside 0..100 or below 100 without last, for a last call that leaves the stream shorter than 9 frames (scipy
 *                          refuses such a clip, and so does artalk_savgol) and for strides that are too small; ARTALK_ESTATE for a session
 *                          whose last call was made already.  Two small table copies and one launch on `stream`: nothing synchronises, no status
 *                          word is published, the workspace is not touched (a lockstep session lives on) and the precision mode plays no
 *                          part.  The state - 9 raw frames in the slot, a frame count on the host - is born with artalk_session_open and
 *                          dropped by whatever closes the session.  Like every call for one model, smooth calls are ordered by the
 *                          caller: the device table of a call is reused by the next one, so two calls on streams that are not ordered
 *                          against each other must not be in flight together. */
int artalk_sessions_reserve(artalk_model* m, int max_sessions);
int artalk_session_open(artalk_model* m, int n, const float* style_motion_dev, const uint8_t* has_style, int64_t* ids_out, void* stream);
int artalk_session_step(artalk_model* m, const int64_t* ids, int n, const float* audio_dev, int64_t chunk_stride, float* out_motion_dev,
                        int64_t out_stride, uint8_t* out_bits_dev, uint8_t* out_hist_bits_dev, void* stream);
int artalk_session_close(artalk_model* m, const int64_t* ids, int n);
int artalk_session_count(const artalk_model* m);
int artalk_session_smooth(artalk_model* m, const int64_t* ids, int n, const float* raw_dev, int64_t raw_stride, const int* n_frames,
                          const uint8_t* last, float* out_dev, int64_t out_stride, int* first_out, int* count_out, void* stream);

/* FLAME linear blend skinning: the consumer behind BITWISE_VAE.get_flame_verts (bitwise_vae.py:43-57) ->
 * FLAMEModel.forward(no_lmks=True) (app/flame_model/FLAME.py:117-142) -> lbs (app/flame_model/lbs.py:142-233).  Host arrays in
 * the layouts of the reference's buffers: v_template [V][3], shapedirs [V][3][NB], posedirs_t [V*3][36] (the reference buffer
 * transposed), J_regressor [5][V], parents [5], lbs_weights [V][5].  artalk_flame_verts: betas_dev [T][NB] (shape ++ expression),
 * full_pose_dev [T][15] (global, neck, jaw, eyes) -> out_dev [T][V][3], already multiplied by `scale`. */
typedef struct artalk_flame artalk_flame;
int artalk_flame_create(int device_id, int V, int NB, int P, const float* v_template, const float* shapedirs, const float* posedirs_t,
                        const float* J_regressor, const int32_t* parents, const float* lbs_weights, float scale, artalk_flame** out);
int artalk_flame_verts(artalk_flame* f, const float* betas_dev, const float* full_pose_dev, int T, float* out_dev, void* stream);
void artalk_flame_destroy(artalk_flame* f);
const char* artalk_flame_last_error(const artalk_flame* f);

/* FLAME mesh renderer: a stand-in for RenderMesh.forward (app/flame_model/renderer_utils.py:55-85), which wraps pytorch3d's
 * rasteriser (blur_radius 0, one face per pixel, no back-face culling, perspective-correct barycentrics) and HardPhongShader.  What
 * is computed is defined in DESIGN.md ("Mesh renderer"); parity with pytorch3d itself is unpinned (no pytorch3d build to compare with).
 * artalk_render_create: faces_host [F][3] vertex indices in [0, V), image_size in 1..16384, scale as RenderMesh's (default camera at
 * distance 2 * scale).  ARTALK_EINVAL with a message (artalk_render_last_error(NULL)) before the device is touched for V <= 0, F <= 0,
 * a bad image_size, a NULL faces_host / out or a face index outside [0, V).
 * artalk_render_mesh: verts_dev [T][V][3] fp32 world space -> rgb_dev [T][3][S][S] in 0..255 (255 where no face covers the pixel),
 * alpha_dev [T][1][S][S] 0 or 1, pix_to_face_dev_or_null [T][S][S] (-1 for background; for tests and debugging).
 * transform_3x4_host_or_null: row-major M with R = M[:, :3], T = M[:, 3] (p_view = p_world . R + T), NULL = diag(-1, 1, -1) and
 * (0, 0, 2 * scale); focal_or_0: focal length in NDC units, 0 = 12.  Runs on the caller's stream and does not synchronise; bit-identical
 * from run to run and for any split of the frames over calls.  ARTALK_EINVAL for a NULL handle, NULL verts / rgb / alpha or T < 0;
 * T == 0 succeeds and does nothing.
 * artalk_render_set_slab: frames per pass over the key buffer (8 bytes per pixel and frame); 0 = the default chosen at create time (32 MiB
 * of keys, at most 64 frames), which is also the largest value accepted.  Returns the value in force. */
typedef struct artalk_mesh_renderer artalk_mesh_renderer;
int artalk_render_create(int device_id, int V, int F, const int32_t* faces_host, int image_size, float scale, artalk_mesh_renderer** out);
int artalk_render_mesh(artalk_mesh_renderer* r, const float* verts_dev, int T, const float* transform_3x4_host_or_null, float focal_or_0,
                       float* rgb_dev, float* alpha_dev, int32_t* pix_to_face_dev_or_null, void* stream);
int artalk_render_set_slab(artalk_mesh_renderer* r, int frames);
void artalk_render_destroy(artalk_mesh_renderer* r);
const char* artalk_render_last_error(const artalk_mesh_renderer* r);

/* Gaussian splat rasteriser, forward only, 32 channels: a stand-in for the CUDA extension diff_gaussian_rasterization_32d that the
 * reference's GAGAvatar head calls under torch.no_grad (app/GAGAvatar/utils_renderer.py:6, models.py:63).  What is computed is defined in
 * DESIGN.md ("Gaussian splat rasteriser"): the 3D-Gaussian-splatting forward pass with precomputed colours and 16 x 16 tiles; parity with
 * the CUDA extension itself is unpinned (neither its source nor a build of it to compare with).  No spherical harmonics, no backward.
 * artalk_splat_render: T frames of N Gaussians onto H x W.  The five attribute arrays are device fp32: means [N][3], colors [N][32],
 * opacities [N], scales [N][3], rotations [N][4] as (r, x, y, z), used as given; each comes with the number of ELEMENTS between two
 * frames, 0 = one set shared by all frames.  view_host / proj_host: n_cams (1 or T) row-major 4 x 4 matrices in HOST memory, row-vector
 * convention ((p, 1) . V), read before the call returns.  bg_dev_or_null: 32 device floats, NULL = zeros.  out_dev [T][32][H][W],
 * radii_dev [T][N] int32 (0: culled).  Every pixel and every radius is written; nothing else is.
 * Unlike the rest of this interface the call WAITS ONCE on `stream`: the number of (tile, Gaussian) pairs depends on the data, so after a
 * counting pass the host reads the frames' pair counts and grows the sort buffers (the CUDA extension does the same); artalk_model's
 * no-synchronisation rule does not bind this object.  Growing a buffer waits for the device too; a repeated shape allocates nothing.
 * Bit-identical from run to run and for any split of the frames over calls.
 * ARTALK_EINVAL with a message, before the device is touched: a NULL handle (artalk_splat_last_error(NULL)), N < 0, T < 0, H or W outside
 * 1..4096, n_cams not 1 or T, a tanfov that is not positive, a negative stride, NULL out, and with N > 0 a NULL attribute, matrix or
 * radii pointer.  T == 0 succeeds and does nothing; N == 0 writes the background.  ARTALK_EHIP: an allocation failed (the message names
 * the size); ARTALK_ECAPACITY: one frame has more than 2^31 - 1 pairs.  artalk_splat_create only refuses a NULL out or a negative
 * device_id; the device is first touched by a render call that passes its checks.  One handle serves any shape; it must not be used
 * from two threads at once.
 * artalk_splat_set_timing / artalk_splat_get_timing (tools/splat_bench.py): with timing on, a call records HIP events around its stages and
 * waits for them at its end; get_timing copies up to n of the 6 per-stage sums in ms (count pass, preprocess, scan + emit, sort, ranges,
 * blend) of the last call, its pairs and frames (each nullable), and returns 6.
 * artalk_splat_render_sets: artalk_splat_render for attributes that lie in pools of sets (resident avatars).  set_of_frame_host: T host
 * int32, frame t's set in [0, n_sets), read before the call returns; each attribute comes with the number of ELEMENTS between two sets,
 * and frame t's attribute starts at base + set[t] * set stride + t * frame stride (a frame stride of 0 as above; a set stride of 0: no
 * pool).  A colour set stride need not be a multiple of 4 floats: the 16-byte test is made on every frame's colour pointer.  Same
 * wait, same bits: frame t equals artalk_splat_render of one frame on that frame's attributes.  set_of_frame_host == NULL is
 * artalk_splat_render.  ARTALK_EINVAL in addition: a negative set stride, a set outside [0, n_sets). */
typedef struct artalk_splat artalk_splat;
int artalk_splat_create(int device_id, artalk_splat** out);
int artalk_splat_render(artalk_splat* s, int N, int T, int H, int W, const float* means_dev, int64_t means_stride, const float* colors_dev,
                        int64_t colors_stride, const float* opacities_dev, int64_t opacities_stride, const float* scales_dev,
                        int64_t scales_stride, const float* rotations_dev, int64_t rotations_stride, const float* view_host,
                        const float* proj_host, int n_cams, float tanfovx, float tanfovy, float scale_modifier, const float* bg_dev_or_null,
                        float* out_dev, int32_t* radii_dev, void* stream);
int artalk_splat_render_sets(artalk_splat* s, int N, int T, int H, int W, const float* means_dev, int64_t means_stride, const float* colors_dev,
                             int64_t colors_stride, const float* opacities_dev, int64_t opacities_stride, const float* scales_dev,
                             int64_t scales_stride, const float* rotations_dev, int64_t rotations_stride, const float* view_host,
                             const float* proj_host, int n_cams, float tanfovx, float tanfovy, float scale_modifier,
                             const float* bg_dev_or_null, float* out_dev, int32_t* radii_dev, const int32_t* set_of_frame_host, int n_sets,
                             int64_t means_set_stride, int64_t colors_set_stride, int64_t opacities_set_stride, int64_t scales_set_stride,
                             int64_t rotations_set_stride, void* stream);
int artalk_splat_set_timing(artalk_splat* s, int enable);
int artalk_splat_get_timing(const artalk_splat* s, double* stage_ms, int n, long long* pairs, int* frames);
void artalk_splat_destroy(artalk_splat* s);
const char* artalk_splat_last_error(const artalk_splat* s);

/* StyleUNet upsampler of the GAGAvatar head, forward only, exact fp32 by default (precision modes below): a stand-in for StyleUNet(in_size = out_size)
 * (app/GAGAvatar/modules/style_unet.py), the consumer of the splat image.  What is computed is defined in DESIGN.md ("StyleUNet
 * upsampler").  Checked on synthetic weights only; parity on real GAGAvatar checkpoints is unpinned.
 * artalk_styleunet_create: out_size a power of two in 8..1024, in_dim / out_dim in 1..4096; host work only (the device is first touched by
 * finalize).  ARTALK_EINVAL with a message (artalk_styleunet_last_error(NULL)) otherwise.
 * artalk_styleunet_set_tensor: one entry of the reference module's state_dict(), fp32 in host memory, with exactly its name and shape
 * (the dead toRGB.* parameters and the stylegan_decoder.noises.noise{i} buffers included).  ARTALK_EKEY "Unexpected key in state_dict: K",
 * ARTALK_EINVAL "size mismatch for K", ARTALK_ESTATE after finalize.
 * artalk_styleunet_finalize: ARTALK_EMISSING "Missing key(s) in state_dict: ..." (the first 8); otherwise packs the weights, uploads them
 * and allocates the workspace for the default slab.
 * artalk_styleunet_forward: x_dev [B][in_dim][S][S] -> out_dev [B][out_dim][S][S], sigmoid applied when activation != 0.
 * noise_ptrs_or_null: host array of num_layers = 2 log2(S) - 3 device pointers, layer l holding [B or 1][r][r] with r = 2^((l + 5) / 2);
 * noise_batch_strides: elements between two samples per layer, 0 = one image for all samples.  NULL = the stored noise buffers.
 * Runs on the caller's stream without synchronising, in slabs of frames; bit-identical from run to run and for any split of the frames
 * over slabs and calls.  ARTALK_ESTATE before finalize; ARTALK_EINVAL before the device is touched for a NULL handle, x or out, B < 0, a
 * NULL noise pointer or stride array, or a stride that is neither 0 nor at least r * r.  B == 0 succeeds and does nothing.
 * artalk_styleunet_set_slab: frames per pass over the workspace; 0 = the default chosen at create time (4 GiB of workspace, at most 64
 * frames), which is also the largest value accepted.  Returns the value in force.
 * artalk_styleunet_set_timing / get_timing (tools/styleunet_bench.py): with timing on, a call times its conv launches with event pairs
 * and WAITS at its end; get_timing returns the summed conv kernel time and the whole call's time of the last call, in ms;
 * get_launch_timing returns the number of conv launches of the last timed call and fills, for the first n of them in launch order,
 * launch_ms[i] and geometry[5 i ..] = frames, H (= W), Cin, Cout, k (either array may be NULL).
 * artalk_op_conv2d: one launch of the conv kernel on CHANNELS-LAST tensors.  x [B][H][W][Cin] (x_bstride elements between samples, 0 =
 * one image for all), w [k k][Cin][Cout] (k = 1 or 3, stride 1, zero padding k / 2), out [B][H][W][Cout].  Prologue: in_scale [B][Cin].
 * Epilogue, each part optional (NULL / gain 1 / lrelu 0), in this order: out_scale [B][Cout], gain, + noise_weight[0] *
 * noise [B or 1][H][W] (noise_bstride 0 = shared), + bias [Cout], LeakyReLU 0.2, * sft_scale + sft_shift and + residual (all
 * [B][H][W][Cout]).  artalk_op_resample2: channels-last bilinear x2 (up != 0) or x0.5 (H, W even), align_corners = False.
 * Precision modes of the convolutions ("Precision modes"): 0 = f32 (the default, exact fp32), 1 = bf16x3 (operands
 * split into bf16 hi + lo, three products on v_mfma_f32_32x32x16_bf16: within a few 1e-5 of fp32 on the synthetic weights), 2 = bf16 (one
 * product: a throughput mode, several 8-bit grey levels off at out_size 64).  Accumulation and the epilogue stay fp32, and everything
 * that is not a convolution keeps its kernels; bf16 has fp32's exponent range, so no mode needs scales, calibration or a range guard.
 * artalk_styleunet_set_precision: ARTALK_EINVAL for a NULL handle or an unknown mode.  Before finalize the mode is only remembered (host
 * work only); after finalize the first selection of a non-zero mode packs the conv weights on the device (+4 bytes per conv weight,
 * waits for the device once) - a module that never selects one allocates nothing.  Switching changes neither the handle nor the
 * workspace nor the slab, results stay bit-identical from run to run and for any split of the frames in every mode, and mode 0 gives
 * the bits it gave before.  artalk_styleunet_get_precision: the mode in force, or ARTALK_EINVAL for a NULL handle.
 * artalk_op_conv2d_ex: artalk_op_conv2d with a precision argument, from the same fp32 weights; precision 0 IS artalk_op_conv2d.  In modes
 * 1 and 2 it packs the weight into a block it owns, on the caller's stream, WAITS for that stream and frees the block.  Every refusal
 * (an unknown precision included) comes before the device is touched.
 * artalk_op_conv2d_plan: which kernel instantiation artalk_op_conv2d_ex runs for these arguments and on what grid - plan_conv, the one host
 * function launch_conv and launch_conv_bf16 switch on, asked without a device.  x_addr, w_addr and in_scale_addr (0: no input scale) are
 * addresses that are looked at for presence and 16-byte alignment and never dereferenced.  Fills out[0 .. min(n, 9)) with NT (1: Cout <=
 * 32, else 2), VA (1: vector loads of x and in_scale - Cin % 8 == 0, x and in_scale 16-byte aligned, x_bstride % 4 == 0), VB (fp32: 1 for
 * vector loads of w - Cout % 4 == 0 and w 16-byte aligned; -1 in modes 1 and 2, which read the packed copy), NP (products per step: 0 fp32,
 * 3 bf16x3, 1 bf16), grid x (128-pixel tiles), grid y (32 NT-channel tiles), the K steps of the main loop, and the packed weight's Cinp
 * and Kp (0 in fp32): conv_mfma_kernel<NT, VA, VB> or conv_bf16_kernel<NT, NP, VA>.  Returns 9, the number of values, or ARTALK_EINVAL
 * for what artalk_op_conv2d_ex refuses in these arguments (and for n < 0, or n > 0 with a NULL out).  Host work only. */
typedef struct artalk_styleunet artalk_styleunet;
int artalk_styleunet_create(int device_id, int in_dim, int out_dim, int out_size, artalk_styleunet** out);
int artalk_styleunet_set_tensor(artalk_styleunet* u, const char* key, const void* host_ptr, int ndim, const int64_t* shape);
int artalk_styleunet_finalize(artalk_styleunet* u);
int artalk_styleunet_forward(artalk_styleunet* u, const float* x_dev, int B, const float* const* noise_ptrs_or_null,
                             const int64_t* noise_batch_strides, int activation, float* out_dev, void* stream);
int artalk_styleunet_set_slab(artalk_styleunet* u, int frames);
int artalk_styleunet_set_timing(artalk_styleunet* u, int enable);
int artalk_styleunet_get_timing(const artalk_styleunet* u, double* conv_ms, double* total_ms);
int artalk_styleunet_get_launch_timing(const artalk_styleunet* u, double* launch_ms, int32_t* geometry, int n);
void artalk_styleunet_destroy(artalk_styleunet* u);
const char* artalk_styleunet_last_error(const artalk_styleunet* u);
int artalk_op_conv2d(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                     const float* in_scale, const float* out_scale, float gain, const float* noise, int64_t noise_bstride,
                     const float* noise_weight, const float* bias, int lrelu, const float* sft_scale, const float* sft_shift,
                     const float* residual, void* stream);
int artalk_styleunet_set_precision(artalk_styleunet* u, int mode);
int artalk_styleunet_get_precision(const artalk_styleunet* u);
int artalk_op_conv2d_ex(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                        const float* in_scale, const float* out_scale, float gain, const float* noise, int64_t noise_bstride,
                        const float* noise_weight, const float* bias, int lrelu, const float* sft_scale, const float* sft_shift,
                        const float* residual, int precision, void* stream);
int artalk_op_conv2d_plan(uint64_t x_addr, int64_t x_bstride, uint64_t w_addr, uint64_t in_scale_addr, int B, int H, int W, int Cin, int Cout,
                          int k, int precision, int32_t* out, int n);
int artalk_op_resample2(const float* x, float* out, int B, int H, int W, int C, int up, void* stream);

/* The style path and layout kernels of the StyleUNet alone, one launch each through the launcher (and so the grid) the network uses, on
 * the given stream, without waiting.  All arrays are dense float32 on the device.  ARTALK_EINVAL for a NULL required pointer, a
 * non-positive dimension or ld < Cin, before the device is touched.
 * su_linear:    y [B][Out] = act(x [B][In] . W [Out][In] + bias [Out] (NULL: none)); lrelu != 0: LeakyReLU 0.2 after the bias.
 * su_normstyle: y [B][n] = x [B][n] * rsqrt(mean over n of x^2 + 1e-8), row by row (NormStyleCode).
 * su_demod:     d [B][Cout] = rsqrt(sum over ci of s[b][ci]^2 * wsq [Cout][Cin] + 1e-8); row b of s starts at s + b * ld, ld >= Cin.
 * su_add:       out [n] = a [n] + b [n].
 * su_to_nhwc:   x [B][C][HW] -> out [B][HW][C].
 * su_to_nchw:   x [B][HW][C] -> out [B][C][HW], through 1 / (1 + exp(-v)) when sigmoid != 0. */
int artalk_op_su_linear(const float* x, const float* W, const float* bias_or_null, float* y, int B, int In, int Out, int lrelu, void* stream);
int artalk_op_su_normstyle(const float* x, float* y, int B, int n, void* stream);
int artalk_op_su_demod(const float* s, int64_t ld, const float* wsq, float* d, int B, int Cin, int Cout, void* stream);
int artalk_op_su_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int artalk_op_su_to_nhwc(const float* x, float* out, int B, int C, int64_t HW, void* stream);
int artalk_op_su_to_nchw(const float* x, float* out, int B, int C, int64_t HW, int sigmoid, void* stream);

/* Read-only views of a handle, for objects that borrow it (artalk_gaga below).  Both return the handle's device index, or ARTALK_EINVAL for
 * a NULL handle; every out pointer may be NULL.  artalk_styleunet_dims: *finalized is 1 after artalk_styleunet_finalize, *slab is the
 * slab in force. */
int artalk_flame_dims(const artalk_flame* f, int* V, int* NB, float* scale);
int artalk_styleunet_dims(const artalk_styleunet* u, int* in_dim, int* out_dim, int* out_size, int* finalized, int* slab);

/* The per-frame path of the GAGAvatar head: motion codes -> RGB frames, a stand-in for GAGAvatar.build_forward_batch + forward_expression
 * (app/GAGAvatar/models.py:63-138).  What is computed is defined in DESIGN.md section 5 ("GAGAvatar head").  The identity side (DINOv2, the
 * Gaussian generators) runs once per avatar elsewhere (the generators: artalk_gsgen_* below); its result, the avatar's Gaussians, comes in
 * as data.
 * artalk_gaga_create: borrows a FLAME handle (V vertices, NB betas, built with scale 5), a splat rasteriser and a StyleUNet (32 -> 3 channels
 * at S x S), all on `device_id` and all outliving this object.  ARTALK_EINVAL with a message (artalk_gaga_last_error(NULL)) for a NULL handle
 * or out, NB < 100, or V / NB / S that are not the borrowed handles'.  With V > 3913 the forehead indices are the reference's 68.
 * artalk_gaga_set_avatar: host fp32 arrays xyz [N][3] (its first V rows are ignored: those Gaussians ride on the vertices), colors [N][32],
 * opacities [N], scales [N][3], rotations [N][4], shapecode [NB - 100], transform [3][4] = [R | t]; uploaded once.  N >= V.  The EMA state
 * is NOT touched (the reference's set_avatar_id does not touch it either).
 * artalk_gaga_set_forehead: K distinct vertex indices in [0, V) whose positions are smoothed over frames (state = 0.98 state + 0.02
 * current, the first frame ever taken as it is); K = 0 switches the smoothing off.  Resets the state.  artalk_gaga_reset_state unsets it.
 * artalk_gaga_set_watermark: host rgba [4][h][w] with h, w <= S, blended into the bottom-right corner (p = p (1 - 0.8 alpha) + rgb 0.8 alpha);
 * NULL removes it.
 * artalk_gaga_set_slab: frames per pass over the head's own scratch (means, radii, splat image, vertices); 0 = the default, what fits
 * 512 MiB, at most 64.  The value in force, which is returned, is never larger than the StyleUNet's slab in force.
 * artalk_gaga_render: motion_dev [T][>= 106] device fp32 with motion_stride elements between rows (not modified) -> out_dev [T][3][S][S]
 * in [0, 1].  Per slab: FLAME inputs -> artalk_flame_verts -> forehead EMA -> means -> artalk_splat_render (per-frame cameras from
 * artalk_gaga_cameras, the avatar's attributes shared by all frames, zero background, tanfov 1 / 12) -> artalk_styleunet_forward
 * (activation and noise arguments as there; the slab's slice of a per-frame noise) -> clamp and watermark.  WAITS on `stream` once for the
 * T head-rotation codes (the cameras are built on the host), and the splat call waits once more in every slab; the scratch grows
 * (and waits) on the first call of a size.  Bit-identical from run to run and for any split of the frames over slabs and calls (the EMA
 * state carries over).  T == 0 succeeds and does nothing.  ARTALK_EINVAL with a message before the device is touched: a NULL handle, motion
 * or out, T < 0, motion_stride < 106, no avatar set, a bad noise argument; ARTALK_ESTATE: the upsampler is not finalized.
 * artalk_gaga_set_timing / get_timing (tools/gaga_bench.py): with timing on a call records HIP events around its stages and waits at its
 * end; get_timing copies up to n of the 5 per-stage sums in ms (inputs + FLAME, forehead + means, splat, upsampler, finish), returns 5.
 * artalk_gaga_cameras (host only): T rotation codes (rot_stride >= 3 floats apart) and the avatar's transform -> view_out / proj_out
 * [T][16] as artalk_splat_render reads them, and cam_out_or_null [T][12] = the frame's [M | t] with M = diag(-1, 1, -1) . exp([w]x)^T,
 * w = (-r0, r1, -r2), t the avatar's own; evaluated in double, rounded once.
 * artalk_op_gaga_*: one launch of one kernel on device arrays.  flame_inputs: -> betas [T][NB], pose [T][15].  forehead: verts [T][V][3] in
 * place, idx [K], state [K][3] and *flag in / out.  means: verts [F][V][3], xyz [N][3] -> means [F][N][3].  finish: img [F][3][S][S] in
 * place, rgba [4][h][w] or NULL.  artalk_op_gaga_check (host only): the checks of set_avatar, set_forehead, set_watermark (skipped when
 * wm_h = wm_w = 0) and render, in this order, on plain numbers; returns the first failing code and copies its message. */
typedef struct artalk_gaga artalk_gaga;
int artalk_gaga_create(int device_id, artalk_flame* flame, artalk_splat* splat, artalk_styleunet* unet, int V, int NB, int S, artalk_gaga** out);
int artalk_gaga_set_avatar(artalk_gaga* g, int N, const float* xyz, const float* colors, const float* opacities, const float* scales,
                           const float* rotations, const float* shapecode, const float* transform_3x4);
int artalk_gaga_set_forehead(artalk_gaga* g, const int32_t* idx, int K);
int artalk_gaga_set_watermark(artalk_gaga* g, const float* rgba_host, int h, int w);
int artalk_gaga_reset_state(artalk_gaga* g);
int artalk_gaga_set_slab(artalk_gaga* g, int frames);
int artalk_gaga_render(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const float* const* noise_ptrs_or_null,
                       const int64_t* noise_batch_strides, int activation, float* out_dev, void* stream);
int artalk_gaga_set_timing(artalk_gaga* g, int enable);
int artalk_gaga_get_timing(const artalk_gaga* g, double* stage_ms, int n);
void artalk_gaga_destroy(artalk_gaga* g);
const char* artalk_gaga_last_error(const artalk_gaga* g);
int artalk_gaga_cameras(const float* rot_host, int64_t rot_stride, int T, const float* transform_3x4_host, float* view_out, float* proj_out,
                        float* cam_out_or_null);
int artalk_op_gaga_flame_inputs(const float* motion_dev, int64_t motion_stride, const float* shapecode_dev, int NB, int T, float* betas_dev,
                                float* pose_dev, void* stream);
int artalk_op_gaga_forehead(float* verts_dev, const int32_t* idx_dev, int K, int T, int V, float* state_dev, int* flag_dev, void* stream);
int artalk_op_gaga_means(const float* verts_dev, const float* xyz_dev, float* means_dev, int F, int V, int N, void* stream);
int artalk_op_gaga_finish(float* img_dev, int F, int S, const float* rgba_dev_or_null, int h, int w, void* stream);
int artalk_op_gaga_check(int V, int S, int N, const int32_t* idx_host, int K, int wm_h, int wm_w, int T, int64_t motion_stride, int have_avatar,
                         int unet_finalized, char* msg, int msg_cap);

/* Frames out: fp32 planar frames [F][3][H][W] in [0, 1] on the device -> 8-bit frames as a video encoder takes them, a stand-in for the
 * hand-over of inference.py:83-86 and app/utils_videos.py:8-36 (x * 255, .cpu(), astype(uint8), transpose, rgb24 -> yuv420p in the
 * encoder).  What is computed is defined in DESIGN.md section 5 ("Frames out").
 * Quantisation: q(v) = (uint8)(clamp(v, 0, 1) * 255.0f), truncation like astype(np.uint8); NaN -> 0.  The clamp is the one deviation: the
 * reference wraps values outside [0, 1].
 * ARTALK_FRAMES_RGB24: out[f][y][x][c] = q(src[f][c][y][x]), H W 3 bytes a frame (PyAV's "rgb24" from an (H, W, 3) array).
 * ARTALK_FRAMES_YUV420P: BT.601 limited range in integers (>> arithmetic) from the quantised R, G, B: Y = ((66 R + 129 G + 25 B + 128) >> 8)
 * + 16 per pixel; per 2 x 2 block Rm = (R00 + R01 + R10 + R11 + 2) >> 2 (Gm, Bm likewise), U = ((-38 Rm - 74 Gm + 112 Bm + 128) >> 8) + 128,
 * V = ((112 Rm - 94 Gm - 18 Bm + 128) >> 8) + 128.  A frame is Y [H][W], U [H/2][W/2], V [H/2][W/2], contiguous: H W 3 / 2 bytes, the I420
 * frame PyAV's "yuv420p" takes from an (H 3 / 2, W) array and a Y4M file holds.  Parity with libswscale's own rgb24 -> yuv420p (its rounding
 * and chroma filter) is unpinned.
 * artalk_frames_bytes: bytes per frame, or ARTALK_EINVAL (an unknown format, H or W outside 1..16384, yuv420p with an odd H or W).
 * artalk_frames_pack: one launch on `stream`, no wait; src and out need no alignment beyond their element's (the kernel takes its wide
 * path where the addresses allow it and gives the same bytes elsewhere).  Bit-identical from run to run.  F == 0 succeeds and launches
 * nothing.  ARTALK_EINVAL with a message (artalk_frames_last_error) before the device is touched: an unknown format, H or W outside
 * 1..16384, yuv420p with an odd H or W, F < 0, a NULL pointer with F > 0, more than 2^39 groups of four pixels.
 * artalk_op_frames_check (host only): the same checks on plain numbers; returns the code and copies the message.
 * artalk_op_gaga_finish_pack: one launch of the fused kernel artalk_gaga_render_u8 runs: img [F][3][S][S] (not modified), rgba [4][h][w] or
 * NULL -> out [F][artalk_frames_bytes(format, S, S)], byte-equal to artalk_op_gaga_finish followed by artalk_frames_pack.
 * artalk_gaga_render_u8: artalk_gaga_render (arguments, waits, refusals and the forehead EMA exactly as there) with 8-bit frames out:
 * the upsampler writes each slab into fp32 scratch the head owns (allocated on the first such call; the fp32 clip is never
 * materialised) and the fused clamp / watermark / pack kernel writes the slab's frames into out_dev [T][artalk_frames_bytes(format, S, S)].
 * With out_host_or_null (pinned memory, T frames) every slab's bytes are also copied to the host on a copy stream the head owns, behind an
 * event recorded after the slab's pack kernel, so the copy overlaps the next slab; before returning the call makes `stream` wait for the
 * last copy, so that a synchronisation of `stream` covers the host buffer; a call that fails waits for the copies it has started.  ARTALK_EINVAL in addition: an unknown format, yuv420p with an
 * odd S, a NULL out_dev, a `stream` that is being captured. */
#define ARTALK_FRAMES_RGB24 1
#define ARTALK_FRAMES_YUV420P 2
int64_t artalk_frames_bytes(int format, int H, int W);
int artalk_frames_pack(const float* src_dev, int F, int H, int W, int format, uint8_t* out_dev, void* stream);
const char* artalk_frames_last_error(void);
int artalk_op_frames_check(int format, int F, int H, int W, int have_src, int have_out, char* msg, int msg_cap);
int artalk_op_gaga_finish_pack(const float* img_dev, int F, int S, const float* rgba_dev_or_null, int h, int w, int format, uint8_t* out_dev,
                               void* stream);
int artalk_gaga_render_u8(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const float* const* noise_ptrs_or_null,
                          const int64_t* noise_batch_strides, int activation, int format, uint8_t* out_dev, uint8_t* out_host_or_null,
                          void* stream);

/* JPEG out ("JPEG out"): rgb24 frames [F][H][W][3] on the device (what artalk_frames_pack writes) -> one baseline
 * JPEG stream per frame, out_dev [F][cap] and sizes_dev [F], all on the device: what a Motion-JPEG sender puts on the wire.  The stream is
 * defined exactly, in integers: SOI, JFIF 1.1 APP0, two DQT, SOF0 (Y Cb Cr, 4:2:0 or 4:4:4), the four Annex K DHT, DRI = the
 * MCUs of one MCU row, SOS, the scan with RSTn after every MCU row but the last, EOI; full-range BT.601, libjpeg's quality scaling of
 * the Annex K tables.  The header is 629 bytes.  Byte parity with libjpeg is unpinned.
 * artalk_jpeg_default_cap: H W 3 + 1024, enough for any but noise-like pictures at the highest qualities.  artalk_jpeg_bound: enough for
 * every picture: 20 + 63 x 26 bits per block, every byte stuffed, two marker bytes per MCU row, the header.  Both: ARTALK_EINVAL for H or W
 * outside 1..16384 (the bound also for an unknown subsampling).
 * artalk_jpeg_header: the 629 header bytes of a size, quality and subsampling into host memory (host only); returns 629.
 * artalk_jpeg_encode: two launches on `stream` for all F frames, no host wait: every count the host needs is arithmetic on H, W and the
 * subsampling.  sizes[f] = the bytes of frame f's stream at out[f * cap]; a stream that does not fit cap gives sizes[f] = -(the bytes it
 * needs) and its slot's content is unspecified, as are the bytes of a slot behind sizes[f].  Nothing outside [f cap, (f + 1) cap) is
 * written for frame f.  rgb needs no alignment.  Byte-identical from run to run.  The encoder owns its scratch (the worst case of the
 * call's segments, grown by doubling) and one uploaded header per (H, W, quality, subsampling); the first call of a size, and a call that
 * grows scratch, waits for `stream` and is refused while `stream` is being captured.  F == 0 succeeds and launches nothing.
 * ARTALK_EINVAL with a message (artalk_jpeg_last_error; of a NULL encoder: the thread's last message) before the device is touched:
 * quality outside 1..100, an unknown subsampling, H or W outside 1..16384, F < 0 or above 65535, a NULL pointer with F > 0,
 * cap < 629 + 2.  artalk_op_jpeg_check (host only): the same checks on plain numbers; returns the code and copies the message.
 * artalk_jpeg_set_timing (default off; ARTALK_EINVAL for a NULL encoder): events around the two launches; a timed call waits for its last
 * launch.  artalk_jpeg_get_timing: launch_ms[0 .. min(n, 2)) = the rows kernel (colour, DCT, quantisation, entropy coding) and the pack
 * kernel (stuffing, markers, header) of the last timed call; returns 2. */
#define ARTALK_JPEG_420 1
#define ARTALK_JPEG_444 2
typedef struct artalk_jpeg artalk_jpeg;
int64_t artalk_jpeg_default_cap(int H, int W);
int64_t artalk_jpeg_bound(int H, int W, int subsampling);
int artalk_jpeg_header(int H, int W, int quality, int subsampling, uint8_t* out_host, int out_cap);
int artalk_jpeg_create(int device, artalk_jpeg** out);
void artalk_jpeg_destroy(artalk_jpeg* j);
const char* artalk_jpeg_last_error(artalk_jpeg* j);
int artalk_jpeg_encode(artalk_jpeg* j, const uint8_t* rgb_dev, int F, int H, int W, int quality, int subsampling, uint8_t* out_dev, int64_t cap,
                       int64_t* sizes_dev, void* stream);
int artalk_jpeg_set_timing(artalk_jpeg* j, int enable);
int artalk_jpeg_get_timing(const artalk_jpeg* j, double* launch_ms, int n);
int artalk_op_jpeg_check(int F, int H, int W, int quality, int subsampling, int64_t cap, int have_rgb, int have_out, int have_sizes, char* msg,
                         int msg_cap);

/* Live audio in ("Live audio in"): raw PCM packets of any size -> the model's 16 kHz mono blocks, on the device.  A
 * streaming form of torchaudio's Resample(sr, 16000)(x).mean(dim=0) (inference.py:230-231): the 16 kHz samples are bit for bit those of
 * artalk_op_resample_mean on the whole concatenated signal, whatever the packet sizes.  An object of its own, not tied to a model handle.
 * Arithmetic.  Output i = j new + p is sum over k ascending of fmaf(taps[p][k], x_c[j orig - width + k], s), indices outside [0, n)
 * skipped (not added as zeros), then the channels summed in order and divided by (float)nch.  After n_in frames group j is final when
 * j orig + width + orig - 1 < n_in; a push emits exactly the newly final groups, new max(0, floor((n_in - width) / orig)) outputs in all, and
 * end emits the rest up to ceil(new n / orig).  Between pushes a stream keeps the frames from index j_next orig - width on (fewer than
 * ntaps = 2 width + orig a channel, fp32, de-interleaved) in one of two carry buffers that alternate: a launch reads one and writes the other.
 * All counters (frames in, outputs written and taken, ended) are host-side int64; nothing reads the device to learn a count.
 * artalk_pcm_create: `max_streams` rings of ring_blocks x block fp32 samples and their carry buffers, two pinned staging buffers.
 * ARTALK_EINVAL before the device is touched: block < 1, ring_blocks < 2, max_streams outside 1..4096, a ring of 2^30 samples or more.
 * device = ARTALK_PCM_NO_DEVICE: a handle without a device, for tests of the bookkeeping: every call checks, plans and counts as usual,
 * nothing is allocated, copied or launched (packets and out_dev are not read or written).
 * artalk_pcm_set_rate: the tap table [new][2 width + orig] of one sample rate, built by the caller exactly as the whole-clip path builds
 * it (artalk_amd.audio.sinc_resample_kernel; 16 kHz: orig = new = 1, width = 0, one tap of 1.0), uploaded once.  ARTALK_EINVAL: ntaps above
 * ARTALK_PCM_MAX_TAPS, new x ntaps above 2^24, a rate set before with another geometry.
 * artalk_pcm_open: a stream of `channels` (1..8) interleaved channels in `format` (ARTALK_PCM_S16: little-endian int16, value / 32768;
 * ARTALK_PCM_F32) at a rate that has been set; ids are never reused.  ARTALK_ECAPACITY when max_streams are open.
 * artalk_pcm_push: packet i, frames[i] frames at data[i] (host memory, or with on_device device memory that is read in place), for stream
 * ids[i]: ONE launch for all listed streams, whatever their rates.  Host packets and the descriptor table travel in one copy through
 * one of two pinned staging buffers, each guarded by an event: a push waits at most for its own staging buffer to come free.
 * artalk_pcm_end: the stream's signal ends here; emits the outputs that were waiting for frames that will not come.
 * artalk_pcm_available (host arithmetic only): 16 kHz samples written and not yet taken, and whether the stream has ended.
 * artalk_pcm_take: the oldest `block` samples of each listed stream into row i of out_dev (row stride out_stride floats), zero past the
 * stream's last real sample; n_valid_host[i] = the real samples of row i (block, or fewer on the last row of an ended stream).
 * A call is checked whole before anything is enqueued and refused with ARTALK_EINVAL (ARTALK_ESTATE for a push or end after end, and for
 * a take of a stream that has neither a full block nor, ended, at least one sample; ARTALK_ECAPACITY for a push whose outputs would not
 * fit the ring's free space) and nothing changed: an unknown or closed id, an id listed twice, a negative frame count, a NULL packet.
 * Calls of one handle are stream-ordered by the caller; a handle is not thread-safe.  No call synchronises the host with the device
 * except a push whose staging buffer is still in flight or has to grow.
 * artalk_op_pcm_plan (host only): what a push of `frames` frames (end != 0: the end, frames ignored) does to a stream that has taken
 * n_before frames: out[0..5] = outputs emitted, lead (frames before index 0 that the carry does not hold), carry frames in, first frame
 * of the carry out (relative to the carry in's first frame minus lead), carry frames out, groups emitted.
 * artalk_op_pcm_push / artalk_op_pcm_take: one launch of pcm_push_kernel / pcm_take_kernel on the caller's own buffers, for tests: the n
 * descriptors (host memory; the library fills tile_groups / n_tiles) are checked, copied to table_dev (table_bytes >= n x sizeof) and read
 * there by the launch.  artalk_op_pcm_desc_bytes: sizeof the two descriptors (which = 0: push, 1: take). */
#define ARTALK_PCM_S16 1
#define ARTALK_PCM_F32 2
#define ARTALK_PCM_MAX_TAPS 1024
#define ARTALK_PCM_MAX_CHANNELS 8
#define ARTALK_PCM_NO_DEVICE (-1)
typedef struct artalk_pcm artalk_pcm;
typedef struct artalk_pcm_desc {
    const float* taps;        /* [nw][2 width + orig], device                                                                        */
    const void* data;         /* the packet: frames x nch interleaved samples of `format`                                             */
    const float* carry_in;    /* [nch][carry_stride]: carry_n frames a channel                                                        */
    float* carry_out;         /* [nch][carry_stride]: carry_out_n frames a channel, written by the packet's last tile                 */
    float* ring;              /* ring_cap samples                                                                                     */
    int32_t orig, nw, width, nch, format, frames;
    int32_t lead;             /* the span's frame v is the signal's frame v - lead + (first frame of the carry in): v < lead is skipped */
    int32_t carry_n, carry_from, carry_out_n, carry_stride;
    int32_t ring_cap, ring_pos, n_out;      /* output o of the launch goes to ring[(ring_pos + o) % ring_cap]                          */
    int32_t tile_groups, n_tiles;           /* filled by the library                                                                  */
} artalk_pcm_desc;
typedef struct artalk_pcm_take_desc {
    const float* ring;
    int32_t ring_cap, read_pos, n_valid, reserved;
} artalk_pcm_take_desc;
int artalk_pcm_create(int device, int block, int ring_blocks, int max_streams, artalk_pcm** out);
void artalk_pcm_destroy(artalk_pcm* p);
const char* artalk_pcm_last_error(artalk_pcm* p);
int artalk_pcm_set_rate(artalk_pcm* p, int sample_rate, const float* taps_host, int orig, int nw, int width);
int artalk_pcm_open(artalk_pcm* p, int sample_rate, int channels, int format, int64_t* id_out);
int artalk_pcm_close(artalk_pcm* p, int64_t id);
int artalk_pcm_push(artalk_pcm* p, const int64_t* ids, int n, const void* const* data, const int64_t* frames, int on_device, void* stream);
int artalk_pcm_end(artalk_pcm* p, const int64_t* ids, int n, void* stream);
int artalk_pcm_available(artalk_pcm* p, int64_t id, int64_t* samples, int* ended);
int artalk_pcm_take(artalk_pcm* p, const int64_t* ids, int n, float* out_dev, int64_t out_stride, int64_t* n_valid_host, void* stream);
int artalk_op_pcm_plan(int64_t n_before, int64_t frames, int end, int orig, int nw, int width, int64_t* out6);
int artalk_op_pcm_desc_bytes(int which);
int artalk_op_pcm_push(artalk_pcm_desc* descs_host, int n, void* table_dev, int64_t table_bytes, void* stream);
int artalk_op_pcm_take(const artalk_pcm_take_desc* descs_host, int n, void* table_dev, int64_t table_bytes, float* out_dev, int64_t out_stride,
                       int block, void* stream);

/* Live streams through the head ("Live streams through the head"): many independent streams rendered by one call,
 * each frame naming its stream and its avatar.  Nothing here changes artalk_gaga_render / _render_u8, the avatar of
 * artalk_gaga_set_avatar or the EMA state artalk_gaga_reset_state unsets: those stay the classic path's own.
 * Resident avatars.  artalk_gaga_pool_reserve: one device slab per attribute for `slots` avatars of N Gaussians each (all resident avatars
 * share N), every slot empty; the [R | t] transforms stay on the host.  Waits for the device and drops an earlier pool.  ARTALK_EINVAL:
 * a NULL handle, slots outside 1..4096, N < V; ARTALK_ESTATE: a pool exists and a stream is open; ARTALK_EHIP: hipMalloc failed (no pool
 * then).  artalk_gaga_pool_set: fills a slot; arguments and checks of artalk_gaga_set_avatar, and ARTALK_EINVAL for a slot outside the
 * pool (also: no pool reserved) and for an N that is not the pool's.  artalk_gaga_pool_clear empties a slot (ARTALK_EINVAL: a NULL
 * handle, a slot outside the pool).  Overwriting or clearing an occupied slot waits for the device first.
 * Per-stream forehead state.  artalk_gaga_stream_open: *id = a new stream whose state is unset (its first frame is taken as it is); ids
 * count up from 0 and are never reused.  artalk_gaga_stream_reset unsets a stream's state, artalk_gaga_stream_close gives its row of the
 * state pool ([streams][K][3] and [streams] flags on the device, grown by doubling) back.  open and reset wait for the device.
 * ARTALK_EINVAL: a NULL handle or id pointer, an id that was never handed out, a closed stream.  While a stream is open
 * artalk_gaga_set_forehead refuses another K with ARTALK_ESTATE (the same K, other vertices: allowed, the streams' states are kept).
 * artalk_gaga_render_streams: T frames; frame t is rendered from motion row frame_row[t] of motion_dev (row r starts r * motion_stride
 * floats in), with the Gaussians, shapecode and transform of pool slot frame_slot[t] and the EMA state of stream frame_stream[t].  The
 * three lists are HOST arrays of T entries, read before the call returns.  Frames of one stream may lie anywhere in the call; the EMA
 * walks a stream's frames in the order they are listed, reads the state at the stream's first frame of the call and writes it at its
 * last, and carries it across slabs and calls.  A stream may name different slots on different frames (the state is the stream's).
 * format 0: fp32 frames into out_dev [T][3][S][S] (out_u8 and out_host_or_null unused: pass NULL); ARTALK_FRAMES_RGB24 / _YUV420P: 8-bit
 * frames into out_u8 and, with out_host_or_null, to the host as artalk_gaga_render_u8 does it.  Noise, activation, slabs, scratch, the
 * copy stream and the waits are artalk_gaga_render's: one wait for the rotation codes per call, the rasteriser's one per slab.
 * artalk_gaga_streams_slab: the frames per slab this call runs with - artalk_gaga_set_slab's request, else the default for the pool's N
 * (without a pool: what artalk_gaga_set_slab reports) - never more than the StyleUNet's slab in force; ARTALK_EINVAL for a NULL handle.
 * T == 0 succeeds and does nothing.  ARTALK_EINVAL with a message before the device is touched: a NULL handle, motion or out, a NULL
 * list, T < 0, a row below 0, a stream id that was never opened or is closed, a slot outside the pool or empty, motion_stride < 106, a bad
 * noise argument, an unknown format, out_host_or_null with format 0, yuv420p with an odd S, a `stream` that is being captured (8-bit
 * formats); ARTALK_ESTATE: the upsampler is not finalized.  Rows beyond the motion array are the caller's to avoid.
 * artalk_op_gaga_flame_inputs_sets / _forehead_streams / _means_sets: one launch each on device arrays.  flame_inputs_sets: frame_row [T]
 * int64, frame_slot [T], shapecode_pool [slots][NB - 100] -> betas [T][NB], pose [T][15].  forehead_streams: one workgroup per listed
 * stream e < n_streams: its state and flag are row pool_row[e] of state_pool [rows][K][3] / flag_pool [rows] (no row listed twice), its
 * frames frames[offsets[e] .. offsets[e + 1]) index verts [..][V][3] (no frame listed twice) and are walked in this order; a stream with
 * no frames keeps state and flag.  means_sets: xyz_pool [slots][N][3], frame_slot [F] -> means [F][N][3].  Each launches the kernel of
 * the entry point without the suffix, which passes null lists: motion row t, slot 0, one entry over frames 0 .. T-1 on row 0.
 * artalk_op_gaga_streams_check (host only): the checks of pool_reserve (V, pool_slots, pool_N) and render_streams on plain numbers and
 * host arrays - stream_open [n_stream_ids] (1: open) and slot_filled [pool_slots] stand for the handle's books; format 0 skips the frame
 * format's check - returns the first failing code and copies its message. */
int artalk_gaga_pool_reserve(artalk_gaga* g, int slots, int N);
int artalk_gaga_pool_set(artalk_gaga* g, int slot, int N, const float* xyz, const float* colors, const float* opacities, const float* scales,
                         const float* rotations, const float* shapecode, const float* transform_3x4);
int artalk_gaga_pool_clear(artalk_gaga* g, int slot);
int artalk_gaga_stream_open(artalk_gaga* g, int* id);
int artalk_gaga_stream_close(artalk_gaga* g, int id);
int artalk_gaga_stream_reset(artalk_gaga* g, int id);
int artalk_gaga_render_streams(artalk_gaga* g, const float* motion_dev, int64_t motion_stride, int T, const int64_t* frame_row_host,
                               const int32_t* frame_stream_host, const int32_t* frame_slot_host, const float* const* noise_ptrs_or_null,
                               const int64_t* noise_batch_strides, int activation, int format, float* out_dev, uint8_t* out_u8,
                               uint8_t* out_host_or_null, void* stream);
int artalk_gaga_streams_slab(const artalk_gaga* g);
int artalk_op_gaga_flame_inputs_sets(const float* motion_dev, int64_t motion_stride, const int64_t* frame_row_dev, const int32_t* frame_slot_dev,
                                     const float* shapecode_pool_dev, int NB, int T, float* betas_dev, float* pose_dev, void* stream);
int artalk_op_gaga_forehead_streams(float* verts_dev, const int32_t* idx_dev, int K, int V, int n_streams, const int32_t* pool_row_dev,
                                    const int32_t* offsets_dev, const int32_t* frames_dev, float* state_pool_dev, int* flag_pool_dev, void* stream);
int artalk_op_gaga_means_sets(const float* verts_dev, const float* xyz_pool_dev, const int32_t* frame_slot_dev, float* means_dev, int F, int V,
                              int N, void* stream);
int artalk_op_gaga_streams_check(int V, int pool_slots, int pool_N, int T, int64_t motion_stride, const int64_t* frame_row_host,
                                 const int32_t* frame_stream_host, const int32_t* frame_slot_host, const uint8_t* stream_open_host, int n_stream_ids,
                                 const uint8_t* slot_filled_host, int unet_finalized, int format, int S, char* msg, int msg_cap);

/* The Gaussian generators of the GAGAvatar head's identity side, forward only, exact fp32, one avatar per call: a stand-in for
 * LinearGSGenerator, the two ConvGSGenerators, build_points_planes, the direction encoding and the assembly of _gs_params
 * (app/GAGAvatar/models.py:65-87, 141-233, 236-252).  What is computed is defined in DESIGN.md section 5 ("Gaussian generators"); its
 * output is what artalk_gaga_set_avatar takes.  DINOv2 and its DPT head, which produce the two features, are not built.  Checked on
 * synthetic weights only: parity on real GAGAvatar checkpoints is unpinned, and so is the reading of pytorch3d's HarmonicEmbedding.
 * artalk_gsgen_create: V rows of head_base (5023), Dh its width (256), Dg the width of the DINO global vector (768: the normed first patch token, see artalk_dino_forward), C the channels of the
 * feature map (256), P the plane size (296); N = V + 2 P P Gaussians.  Host work only.  ARTALK_EINVAL with a message
 * (artalk_gsgen_last_error(NULL)) for a NULL out, a negative device, (Dh + Dg) % 4 != 0, an odd C, P < 3, or a size outside V 1..2^22,
 * Dh / Dg 1..16384, C 2..4096, P 3..4096.
 * artalk_gsgen_set_tensor: one entry of the reference module's state_dict(), fp32 in host memory, in torch's layout, with exactly its name
 * and shape: head_base, gs_generator_g.feature_layers.{0,2,4,6}.{weight,bias}, gs_generator_g.{color,opacity,scale,rotation}_layers.
 * {0,2}.{weight,bias}, gs_generator_l{0,1}.gaussian_conv.{0,2,4,6}.{weight,bias}.  ARTALK_EKEY "Unexpected key in state_dict: K",
 * ARTALK_EINVAL "size mismatch for K", ARTALK_ESTATE after finalize.
 * artalk_gsgen_finalize: ARTALK_EMISSING "Missing key(s) in state_dict: ..." (the first 8); otherwise transposes the weights on the host,
 * uploads them and allocates the workspace (about 0.3 GB at the reference's sizes).
 * artalk_gsgen_planes (host only): transform [3][4] = [R | t] -> points_out [P P][3] (plane_points, pixel y P + x), dir_out [3],
 * direnc_out [27]; each out pointer may be NULL.  Evaluated in double from the float32 matrix, rounded once.  ARTALK_EINVAL for a NULL or
 * non-finite transform or P outside 3..4096.
 * artalk_gsgen_generate: feature0_dev [C][P][P] and feature1_dev [Dg] on the device, the avatar's transform on the host -> xyz [N][3],
 * colors [N][32], opacities [N], scales [N][3], rotations [N][4] on the device: rows 0 .. V - 1 from the global generator (their xyz
 * zero), rows V + g P P + y P + x from local generator g.  Runs on the caller's stream and does not synchronise; bit-identical from run
 * to run.  ARTALK_ESTATE before finalize; ARTALK_EINVAL before the device is touched for a NULL handle or pointer or a non-finite transform.
 * artalk_gsgen_set_timing / get_timing (tools/gsgen_bench.py): with timing on, a call times its conv launches with event pairs and WAITS
 * at its end; get_timing returns the summed conv kernel time and the whole call's time of the last call, in ms.
 * artalk_gsgen_dims: returns the device index (ARTALK_EINVAL for a NULL handle); every out pointer may be NULL.
 * artalk_op_conv2d_relu: artalk_op_conv2d with only a bias (may be NULL) and the plain ReLU (relu != 0) as its epilogue; with relu == 0
 * it gives artalk_op_conv2d's bits.
 * artalk_op_gs_*: one launch of one kernel on device arrays; direnc and transform are host pointers.  local_input: f_feature0 [C][P][P] ->
 * [P P][W], W = C + 27 rounded up to a multiple of 8, the padding zero (the conv's vector loads).  global_input: head_base [V][Dh],
 * feature1 [Dg] -> [V][Dh + Dg].  concat_dir: feat [V][H] -> [V][W], W = H + 27 rounded up likewise.  local_attr:
 * the 41-channel conv output [P P][41] -> rows row0 .. row0 + P P - 1 of the five avatar arrays, sign +1 (l0) or -1 (l1).  global_attr:
 * the four heads' outputs [V][32], [V], [V][3], [V][4] -> rows 0 .. V - 1 of the five avatar arrays. */
typedef struct artalk_gsgen artalk_gsgen;
int artalk_gsgen_create(int device_id, int V, int Dh, int Dg, int C, int P, artalk_gsgen** out);
int artalk_gsgen_set_tensor(artalk_gsgen* g, const char* key, const void* host_ptr, int ndim, const int64_t* shape);
int artalk_gsgen_finalize(artalk_gsgen* g);
int artalk_gsgen_planes(const float* transform_3x4_host, int P, float* points_out, float* dir_out, float* direnc_out);
int artalk_gsgen_generate(artalk_gsgen* g, const float* feature0_dev, const float* feature1_dev, const float* transform_3x4_host, float* xyz_dev,
                          float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream);
int artalk_gsgen_set_timing(artalk_gsgen* g, int enable);
int artalk_gsgen_get_timing(const artalk_gsgen* g, double* conv_ms, double* total_ms);
int artalk_gsgen_dims(const artalk_gsgen* g, int* V, int* Dh, int* Dg, int* C, int* P, int* finalized);
void artalk_gsgen_destroy(artalk_gsgen* g);
const char* artalk_gsgen_last_error(const artalk_gsgen* g);
int artalk_op_conv2d_relu(const float* x, int64_t x_bstride, const float* w, float* out, int B, int H, int W, int Cin, int Cout, int k,
                          const float* bias, int relu, void* stream);
int artalk_op_gs_local_input(const float* feature0_dev, const float* direnc_host, float* out_dev, int C, int P, void* stream);
int artalk_op_gs_global_input(const float* head_base_dev, const float* feature1_dev, float* out_dev, int V, int Dh, int Dg, void* stream);
int artalk_op_gs_concat_dir(const float* feat_dev, const float* direnc_host, float* out_dev, int V, int H, void* stream);
int artalk_op_gs_local_attr(const float* conv_out_dev, const float* transform_3x4_host, int P, int sign, int64_t row0, float* xyz_dev,
                            float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream);
int artalk_op_gs_global_attr(const float* colors_in_dev, const float* opacities_in_dev, const float* scales_in_dev, const float* rotations_in_dev,
                             int V, float* xyz_dev, float* colors_dev, float* opacities_dev, float* scales_dev, float* rotations_dev, void* stream);

/* DINOBase of the GAGAvatar head's identity side, forward only, exact fp32, one image per call: a stand-in for
 * app/GAGAvatar/modules/dino_base.py - the ImageNet normalisation, the DINOv2 ViT (patch 14, LayerScale, no register tokens), the last
 * four blocks' normed patch tokens and the DPT-style head.  What is computed is defined in DESIGN.md section 5 ("DINO features"); its
 * two outputs are what artalk_gsgen_generate takes.  Checked on synthetic weights only: parity on the real GAGAvatar.pt, the upstream
 * checkpoint's key names and torchvision's resize are unpinned.  Not built: position-embedding interpolation, register tokens, batches,
 * lower-precision modes, only_global / output_size.
 * artalk_dino_create: vit_dim the ViT's width (768), depth its blocks (12), heads (12), grid the patches a side (37: a 518 x 518 image),
 * output_dim the channels of the feature plane (256), whose side is P = 8 grid.  The MLP is 4 vit_dim wide; the head's hidden width 256
 * and projection widths 256 / 512 / 1024 / 1024 are the reference's constants.  Host work only.  ARTALK_EINVAL with a message
 * (artalk_dino_last_error(NULL)) for a NULL out, a negative device, depth < 4, a head width vit_dim / heads other than 64 or 32, vit_dim
 * not a multiple of 32 in 32..4096, grid outside 2..64, output_dim outside 1..1024.
 * artalk_dino_set_tensor: one entry of the reference module's state_dict() (the names under base_model.), fp32 in host memory, in torch's
 * layout: dino_model.{cls_token,pos_embed,mask_token (accepted, unused, may be absent)}, dino_model.patch_embed.proj.*,
 * dino_model.blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.{weight,bias}, dino_model.blocks.N.{ls1,ls2}.gamma,
 * dino_model.norm.*, projects.N.*, resize_layers.{0,1,3}.*, layer_rn.N.weight, refinenet.N.{resConfUnit1,resConfUnit2}.{conv1,conv2}.*
 * (refinenet.0.resConfUnit1 is loaded and never run), refinenet.N.out_conv.*, output_conv.*.  ARTALK_EKEY "Unexpected key in state_dict:
 * K", ARTALK_EINVAL "size mismatch for K" (a pos_embed of another grid: the message says that position embeddings are not interpolated),
 * ARTALK_ESTATE after finalize.
 * artalk_dino_finalize: ARTALK_EMISSING "Missing key(s) in state_dict: ..." (the first 8); otherwise transposes and pads the weights on
 * the host, uploads them and allocates the workspace (about 0.45 GB at the reference's sizes).
 * artalk_dino_prepare_image: image [3][height][width] in host or device memory -> out_dev [3][14 grid][14 grid], torch's antialiased
 * bilinear resize (the reference's build_forward_batch); values are not normalised.  A host image has been read when the call returns (the call
 * waits for its copy); a device image is read on the stream.
 * artalk_dino_forward: image_dev [3][height][width] in [0, 1] on the device -> feature0_dev [output_dim][P][P] and feature1_dev [vit_dim]
 * (the normed first patch token of the last block).  Runs on the caller's stream and does not synchronise; bit-identical from run to run.
 * ARTALK_ESTATE before finalize; ARTALK_EINVAL before the device is touched for a NULL handle or pointer, a non-square image or a size
 * other than 14 grid.
 * artalk_dino_read: after a forward call on the same stream, copies an intermediate to out_dev: "tap0".."tap3" [grid grid][vit_dim] (the
 * normed patch tokens of the last four blocks), "rn0".."rn3" [H H][256] channels-last with H = 4 grid, 2 grid, grid, (grid - 1) / 2 + 1
 * (the layer_rn outputs); n must be the exact count.
 * artalk_dino_set_timing / get_timing (tools/dino_bench.py): with timing on, a forward call marks its stages with events and WAITS at its
 * end; stage_ms [4]: ViT and head GEMMs, attention, the head's convs, everything else.
 * artalk_dino_dims: returns the device index (ARTALK_EINVAL for a NULL handle); every out pointer may be NULL.
 * artalk_op_dino_*: one launch of one kernel on device arrays; ARTALK_EINVAL for a NULL pointer, a size out of range or a misaligned
 * pointer (16 bytes where a channel count must be a multiple of 4).  resize_aa: x [C][Hi][Wi] -> [C][Ho][Wo], or [Ho][Wo][C] with
 * channels_last; normalize (C = 3): the ImageNet mean / std applied to the result.  normalize: [3][n].  im2col: [3][14 g][14 g] ->
 * [g g][608], column c 196 + ky 14 + kx, zeros from 588.  tokens: X[t] = (t ? patch[t - 1] : cls) + pos[t].  layernorm: eps 1e-6,
 * affine, any D % 4 == 0.  strip: [1 + G][D] -> [G][D].  shuffle: the GEMM result [g g][s s Co] of a k = s transposed conv -> [s g][s g][Co]
 * + bias.  gather_s2: [g][g][C] -> [Ho Ho][9 C], the windows of a 3 x 3 stride-2 pad-1 conv.  concat: img [n][3] ++ feat [n][C] ->
 * [n][W], W = 3 + C rounded up to a multiple of 8, the padding zero.  resize_ac: channels-last bilinear, align_corners = True.
 * add_relu: sum = a + b (b NULL: a) to sum_out (may be NULL), max(sum, 0) to relu_out.  output: x [n][C] -> [C][n], and tok [D] -> f1
 * (tok NULL: no). */
typedef struct artalk_dino artalk_dino;
int artalk_dino_create(int device_id, int vit_dim, int depth, int heads, int grid, int output_dim, artalk_dino** out);
int artalk_dino_set_tensor(artalk_dino* d, const char* key, const void* host_ptr, int ndim, const int64_t* shape);
int artalk_dino_finalize(artalk_dino* d);
int artalk_dino_prepare_image(artalk_dino* d, const float* image, int height, int width, float* out_dev, void* stream);
int artalk_dino_forward(artalk_dino* d, const float* image_dev, int height, int width, float* feature0_dev, float* feature1_dev, void* stream);
int artalk_dino_read(artalk_dino* d, const char* what, float* out_dev, int64_t n, void* stream);
int artalk_dino_set_timing(artalk_dino* d, int enable);
int artalk_dino_get_timing(const artalk_dino* d, double* stage_ms, double* total_ms);
int artalk_dino_dims(const artalk_dino* d, int* vit_dim, int* depth, int* heads, int* grid, int* output_dim, int* finalized);
void artalk_dino_destroy(artalk_dino* d);
const char* artalk_dino_last_error(const artalk_dino* d);
int artalk_op_dino_resize_aa(const float* x, float* out, int C, int Hi, int Wi, int Ho, int Wo, int channels_last, int normalize, void* stream);
int artalk_op_dino_normalize(const float* x, float* out, int64_t n, void* stream);
int artalk_op_dino_im2col(const float* img, float* col, int grid, void* stream);
int artalk_op_dino_tokens(const float* patch, const float* cls, const float* pos, float* X, int T, int D, void* stream);
int artalk_op_dino_layernorm(const float* X, float* Y, const float* w, const float* b, int M, int D, void* stream);
int artalk_op_dino_strip(const float* tap, float* out, int G, int D, void* stream);
int artalk_op_dino_shuffle(const float* r, const float* bias, float* out, int grid, int s, int Co, void* stream);
int artalk_op_dino_gather_s2(const float* x, float* col, int grid, int C, void* stream);
int artalk_op_dino_concat(const float* img, const float* feat, float* out, int64_t n, int C, void* stream);
int artalk_op_dino_resize_ac(const float* x, float* out, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
int artalk_op_dino_add_relu(const float* a, const float* b, float* sum_out, float* relu_out, int64_t n, void* stream);
int artalk_op_dino_output(const float* x, float* out, int64_t n, int C, const float* tok, float* f1, int D, void* stream);

/* Numerical health of the work enqueued since the last artalk_infer / artalk_stream_begin started.  Every call ends with an
 * asynchronous copy of the device status word to pinned host memory.  artalk_get_status WAITS for that copy (an event wait:
 * the one synchronisation on this boundary, paid only by callers that ask; `stream` is ignored); artalk_poll_status never
 * blocks and returns ARTALK_EBUSY while the call is still running.  Bits: 0 a logit was NaN/Inf (the pairwise argmax of
 * app/models.py:104 would silently turn it into a 0 bit), 1 a re-encoder output was NaN/Inf, 2 a FLAME code was NaN/Inf,
 * 3 an activation exceeded the range of its site's P8 scale where it was produced (|x| * 2^e > 65504, fp16's largest finite value, or
 * x is NaN; e = the site's exponent, artalk_get_site_scales; |x| > 4094 at the default e = 4: exactly 65504 / 2^e is still stored finite).  Non-zero in f16x3 mode means an activation left fp16's range: the Python
 * host first recalibrates the site scales on that batch (artalk_calibrate) and redoes the call in f16x3 mode; only when nothing could
 * be lowered does it redo the call in f32 mode and stay there. */
int artalk_get_status(artalk_model* m, int* flags, void* stream);
int artalk_poll_status(artalk_model* m, int* flags);
/* Several calls in flight (a serving loop that enqueues batch i+1 before it looks at batch i): every call that publishes a status
 * word gets a ticket (1, 2, ...; artalk_last_ticket right after the call returns it), and artalk_get_status_of waits for THAT call
 * and returns its flags.  The words of the last 4 calls are kept: ARTALK_EINVAL for an older ticket. */
long long artalk_last_ticket(artalk_model* m);
int artalk_get_status_of(artalk_model* m, long long ticket, int* flags);

/* Savitzky-Golay smoothing of inference.py:89-95 on the device: in/out [T][106] f32, T >= 9. */
int artalk_savgol(artalk_model* m, const float* in_dev, float* out_dev, int T, void* stream);

/* Per-call stage timing (HIP events on the call's stream).  level 0 = off; 1 = light: hipGraphs stay on, events
 * bracket the eager launches only (wav2vec2, AdaLN table, graph replays) - cheap enough for a timed region;
 * 2 = full: graphs off, events also inside the AR/VAE body.  artalk_get_profile synchronises and returns the
 * LAST artalk_infer's numbers (milliseconds / counters):
 *   out[0] style  out[1] wav2vec2 conv stack  out[2] wav2vec2 encoder  out[3] AdaLN table GEMM
 *   out[4] AR scale steps (level 1: whole captured body)  out[5] VAE decode+re-encode (level 2 only; + initial history)
 *   out[6] total  out[7] bracketed launches of the dominant kernel (f16x3 mode: gemm_p8_big_kernel, the persistent 320x256 / 256x256-tile
 *   LDS-DMA split GEMM that takes every large GEMM of a step: wav2vec2 q|k|v, out-projection, FFN-in, FFN-out, the feature projection,
 *   conv1-6 and the AdaLN tables; f32 mode: the 128x128-tile fp32 MFMA GEMM)  out[8] their summed ms  out[9] their summed FLOP */
int artalk_set_profiling(artalk_model* m, int level);
int artalk_get_profile(artalk_model* m, double* out, int n);
/* Kernel-time budget without a profiler: after an artalk_infer at profiling level 3 (graphs off, the production clip groups one after the
 * other on one stream, every launch carries its own start / stop events), out[b] = summed kernel durations (ms) per bucket - 0 style, 1 conv stack, 2 encoder, 3 AdaLN tables,
 * 4 history K/V + glue, 5..9 scale steps 0..4, 10 VAE decode, 11 re-encode, 12 other - and out[13] = kernels timed (n >= 14).
 * bench.py reports it next to the stages' event times as `budget_ms`. */
int artalk_get_kernel_sums(artalk_model* m, double* out, int n);
/* GEMM arithmetic: 0 (the library's default; the Python host selects 1) = exact fp32 on v_mfma_f32_32x32x2_f32; 1 = "f16x3": every fp32 operand split into two
 * fp16 values (22 significand bits), three fp16 MFMA products accumulated in fp32 - fp32-class accuracy (parity tests run in
 * both modes) at 5.3x the matrix-core rate; the logit / code heads stay on the fp32 path in both modes.
 * 2 = "bf16", the throughput mode: every GEMM except the logit / code heads computes bf16(A) * bf16(W) with fp32 accumulation
 * (operands rounded to nearest even, one v_mfma_f32_32x32x16_bf16 per product); bias, activation, gate, residual and the split-K
 * reduce stay fp32, and everything else (activations in HBM, LayerNorms, attention, pooling, conv0, quantiser) runs mode 0's
 * schedule - what torch bf16 autocast does to linear / conv.  bf16 has fp32's exponent range: the site scales are not used and
 * status bit 3 is never raised.  The first switch to mode 2 builds a bf16 copy of every weight (+2 bytes per parameter in
 * artalk_weight_bytes); a model that never selects it allocates nothing.  Captured graphs and the cached initial history are kept
 * per mode, so switching back and forth is free and never mixes modes. */
int artalk_set_precision(artalk_model* m, int mode);
/* Replay the AR/VAE part from hipGraphs captured per active-batch size (default 1 = on).  The batch is cut into 1/2/4 clip
 * groups whose graphs run concurrently on separate streams (automatic; enable | (groups << 8) forces a count, for tuning).
 * Bits 16-23 / 24-31, when non-zero, override the split-K policy in units of 16 tiles (split when a GEMM has fewer output
 * tiles than the first, aim for the second; defaults 192 / 384 measured best). */
int artalk_set_graphs(artalk_model* m, int enable);
/* Number of captured body graphs the model holds; *captures (nullable) = captures since the model was created.  The cache is bounded:
 * a group's re-encode count is rounded up to a multiple of 8 and at most 96 executables are kept (least recently used evicted), so a
 * serving loop with ever-changing ragged batches (reference: one clip per call, inference.py:47-57) cannot grow it without limit. */
int artalk_graph_count(const artalk_model* m, long long* captures);
/* Headroom audit of the f16x3 operand format: while enabled every artalk_infer runs without graphs and records, for each
 * producer of a P8 operand (LayerNorm outputs, GEMM results written in P8, attention outputs, ...), max |x| - times the site's scale
 * (16 by default, artalk_get_scales) the value that must stay below fp16's 65504.  Works in both precision modes (in f32 mode the same
 * activations are fp32 buffers).  artalk_get_audit synchronises and returns the number of sites; names_buf receives the site
 * names NUL-separated, values[i] the maximum seen at site i since the audit was switched on (tools/p8_headroom.py). */
int artalk_set_audit(artalk_model* m, int enable);
int artalk_get_audit(artalk_model* m, char* names_buf, int buf_len, float* values, int max_n);
/* Per-site operand scales of the f16x3 format.  Every producer of a P8 operand writes it with a power-of-two scale 2^e and its consumers
 * remove the same scale; e = 4 (x16, range |x| < 4094) by default.  A checkpoint with outlier activations (XLS-R-class encoders: FFN
 * hidden channels of 1e4 and more; the reference loads such a checkpoint, inference.py:24-28) needs more range at a few sites:
 * artalk_calibrate reads the maxima of an audit pass (artalk_set_audit(1) + artalk_infer in EXACT-F32 mode on representative clips)
 * and lowers e at every site where max|x| * 2^e * headroom would exceed fp16's 65504, per site, down to e = -8.  Only those sites change
 * (everything else stays bit-identical); exponents never go up again until artalk_reset_scales.  Returns the number of sites changed,
 * or a negative ARTALK_E* code.  All or nothing: if any site fails (ARTALK_EINVAL: a non-finite maximum, or one no exponent can hold), no
 * exponent changes and the captured graphs are kept.  artalk_get_scales: exps[i] = exponent of audit site i, in the order of artalk_get_audit
 * (first seen during the audit pass: only the sites that ran, so it depends on the clips audited); artalk_*_site_scales below use the
 * fixed table order instead.  The Python host calls this by itself when a call trips the range guard (status bit 3) and re-runs the call
 * in f16x3 mode. */
int artalk_calibrate(artalk_model* m, float headroom);
int artalk_reset_scales(artalk_model* m);
int artalk_get_scales(artalk_model* m, int* exps, int max_n);
/* The site table: every P8 producer site this configuration can run, fixed at artalk_create from the config alone, with the names the
 * audit reports (w2v.layer3.ffn_hidden, ar.block0.ln1_mod, ...).  It is the order a saved calibration is keyed by.  artalk_scale_sites
 * returns the number of sites n and writes their names NUL-separated in table order (names_buf = NULL: only n; a buffer too small:
 * ARTALK_EINVAL).  artalk_get_site_scales writes the n exponents in table order (n must equal the site count).
 * artalk_set_site_scales restores them: n must equal the site count and every exponent must lie in [-8, 4] (what artalk_calibrate
 * can produce), else ARTALK_EINVAL with nothing changed.  Returns the number of sites whose exponent changed; if any did, it
 * synchronises the device, drops the captured graphs and the initial-history cache and ends an open streaming session (the next
 * artalk_stream_chunk fails with ARTALK_ESTATE: a session never mixes exponents).  Setting the values the model holds changes nothing. */
int artalk_scale_sites(const artalk_model* m, char* names_buf, int buf_len);
int artalk_get_site_scales(artalk_model* m, int* exps, int n);
int artalk_set_site_scales(artalk_model* m, const int* exps, int n);
/* Intermediate taps: device buffers that correspond to intermediates of the reference, for parity tests that localise a difference to
 * a kernel group (tests/test_taps_gpu.py against tests/golden/taps_*.npz, captured from the reference by oracle/make_golden_taps.py).
 * While a tap buffer is set, artalk_infer runs the AR/VAE body eagerly as one clip group and copies, for chunk index j and clip
 * position b (clips in the call's sorted order), into slot (j * max_batch + b), as fp32 (artalk_tap_layout gives the field offsets):
 *   blk0_in  [181][768]  attn_feat entering attn_blocks[0], rows of scale step p written at step p        (app/models.py:100)
 *   blk0_out [181][768]  output of attn_blocks[0]                                                          (app/transformer.py:30-43)
 *   blkL_out [181][768]  output of the last block                                                          (app/models.py:101-102)
 *   prev_in  [181][768]  prev_attn_feat + prev_lvl_pos_embed as chunk j uses it                            (app/models.py:101,111-114)
 *   logits   [181][64]   pred_motion_logits, fp32                                                          (app/models.py:103)
 *   dec_out  [200][106]  VAE decoder output before unnorm_with_stats                                       (app/modules/bitwise_vae.py:110-111)
 * With the KV cache only a scale step's NEW tokens are computed, so row t holds the value of the step that introduced token t -
 * which the reference recomputes, bit-identically, in every later step.  tap_dev = NULL switches the taps off. */
int artalk_set_tap(artalk_model* m, float* tap_dev, int max_batch, int max_chunks);
int artalk_tap_layout(int64_t* out, int n);
/* Restrict the model to a set of compute units: bit i of mask[0 .. n_words) = CU i / 8 of XCD i % 8 on MI355X.  The library's own
 * streams get the mask and its persistent kernels size their grids to it; the caller passes a stream created with the same mask
 * (artalk_op_create_masked_stream) to artalk_infer - e.g. to leave compute units to a renderer running beside the path.  (Two
 * replicas of the path on the two halves of the chip measured 18 % BELOW one replica on the whole chip: tools/dual_partition_probe.py,
 * DESIGN.md section 6.)  n_words = 0 clears it.  A stream created with a CU mask (hipExtStreamCreateWithCUMask) is a BLOCKING stream:
 * unlike the library's unmasked side streams (hipStreamNonBlocking) it is implicitly ordered against work on the legacy null stream
 * of the process, and a null-stream call made while the library captures a graph on it is a capture error - keep other GPU work of
 * the process (a renderer) on streams of its own while a partitioned model runs.  The mask count is clamped to the device's CUs. */
int artalk_set_cu_mask(artalk_model* m, const uint32_t* mask, int n_words);

/* ---- single-kernel entry points for the parity tests (device pointers, row-major f32) ---- */
/* C[M,N] = R + gate * act(A[M,K] W[N,K]^T + bias); act: 0 none, 1 gelu(erf), 2 gelu(tanh), 3 leaky_relu(0.2). K % 32 == 0 */
int artalk_op_gemm(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R,
                   float* C, int M, int N, int K, int act, void* stream);
/* same arguments and tiles, K summed in blocks: every 256 of K the running sums are added into a second set and restart from zero.
 * The kernels the DINO object's linear layers run (artalk_dino_forward), for the parity tests at K = 768 and 3072. */
int artalk_op_gemm_blocked(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R,
                           float* C, int M, int N, int K, int act, void* stream);
/* same, with an explicit tile configuration (4: 128x128 BK16, 2: 64x64, 1: 128x64, 3: 32x128; -1: heuristic) for tuning */
int artalk_op_gemm_ex(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                      int force_cfg, void* stream);
/* calibration: register-only fp32 MFMA loop (blocks x 256 threads, 32*iters MFMAs per wave, nacc = 1 or 4 independent accumulators); *flops = FLOPs of the launch */
int artalk_op_mfma_f32_peak(float* out_dev, int blocks, int iters, int nacc, double* flops, void* stream);
/* f16x3 split GEMM (mode 1 above) on fp32 inputs; cfg 0: 128x128 tiles, 1: 64x64, -1: heuristic.  M > 32, K % 32 == 0 */
int artalk_op_gemm_f16s(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                        int force_cfg, void* stream);
/* bf16 GEMM on fp32 inputs (W converted to bf16 internally): C[m, n] = R + gate * act(bf16(A) bf16(W)^T + bias), ldc = ldg = ldr = N,
 * K % 32 == 0, lda % 4 == 0 (lda < K: a convolution window), A and W 16-byte aligned.  force_cfg -1 = the engine's tile choice; otherwise
 * bits 0-7 select the tile of the register-staged gemm_bf16_kernel (0: 64x64, 1: 128x128, 2: 32x128, 0xff: engine's choice), bits 8-15 a split-K factor (finished
 * by the split-K reduce pass), bits 16-23 a grid.z batch (batch z at A + z*M*lda, W + z*N*K, bias + z*N, R / C + z*M*N), bit 24 the
 * grouped positional-conv window (amode 1: 64 input channels per group at A + z*64, taps = K / 64, pad = taps / 2, clips of T = bits
 * 25-30 rows).  Synchronises the stream. */
int artalk_op_gemm_bf16(const float* A, int64_t lda, const float* W, const float* bias, const float* gate, const float* R, float* C,
                        int M, int N, int K, int act, int force_cfg, void* stream);
/* tuning helpers: fp32 -> packed split words; split GEMM on pre-packed W (and optionally pre-packed A).  force_cfg -1 / 0 / 1: the
 * register-staged kernel (heuristic / 128x128 / 64x64); with a_packed the LDS-DMA kernels of the f16x3 planner: 7 / 12 = gemm_p8_big_kernel
 * (256x256 / 320x256 tiles), 8 = gemm_p8_2wgp_kernel (a forced 7 / 12 / 8 the shape cannot take falls back: 7 / 12 to 8, 8 to the plan),
 * 20 / 23 / 24 = gemm_p8_sm_kernel (64x64, 4 / 8 / 5 stages), 28 = gemm_p8_mid_kernel, 31 = gemm_p8_pp_kernel; for 20 .. 31 bits 8-15
 * are a split-K factor and bit 16 fetches the weights non-temporally; 99 = the planner's own choice (no split-K).  Retired values run
 * what replaced them: 13 as 99, 29 and 33 as 28, 30 as 31.  Other values, and a split factor above K / 32 (a workgroup would own no
 * K step): EINVAL before anything is allocated. */
int artalk_op_pack_split(const float* in, void* out_u32, int64_t n, int is_weight, void* stream);   /* operand scale: 0 activation, 1 weight */
int artalk_op_gemm_f16s_packed(const void* A, int a_packed, int64_t lda, const void* Wp, const float* bias, float* C, int M, int N,
                               int K, int act, int force_cfg, void* stream);
/* frees the split-K scratch artalk_op_gemm_f16s_packed grows on demand (the buffers it outgrew are kept until this call, because
 * graphs captured from earlier launches still write to them): call it when no such graph will be replayed again */
int artalk_op_release_scratch(void);
/* which production LDS-DMA kernel the f16x3 planner picks for an M x N x K product (dense rows, with or without a residual) with both
 * operands in P8 and no forced configuration (what the model path calls): on a large grid 7 / 12 = gemm_p8_big_kernel with 256x256 /
 * 320x256 tiles, 8 = gemm_p8_2wgp_kernel; otherwise the small-grid configuration without split-K (20, 28, 31: see
 * artalk_op_gemm_f16s_packed); force_cfg 99 of artalk_op_gemm_f16s_packed launches exactly that choice */
int artalk_op_gemm_p8_plan(int M, int N, int K, int residual);
/* a HIP stream restricted to the compute units whose bits are set in mask[0 .. n_words) (hipExtStreamCreateWithCUMask; on MI355X bit i =
 * CU i / 8 of XCD i % 8): the stream a model with artalk_set_cu_mask is driven on */
int artalk_op_create_masked_stream(const uint32_t* mask, int n_words, void** out_stream);
int artalk_op_destroy_stream(void* stream);
/* y = LN(x)[*w+b][*(1+scale)+shift][act], D in {128,512,768,1024}; act | 0x100 writes y in the P8 split format */
int artalk_op_layernorm(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift,
                        int M, int D, float eps, int act, void* stream);
/* Q,K,V,O: [B][L][H*HD] contiguous; l2norm bit 0 -> q,k normalised, q *= qscale[h]; bit 1 -> the fp16 operand-split kernel of
 * f16x3 mode (HD = 64); bit 2 (with bit 1, without bit 0) -> Q, K, V are given in the P8 split format; split: queries<split see keys<split */
int artalk_op_attention(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                        float scale, int l2norm, const float* qscale, int split, void* stream);
/* audio [C][n] -> normalised -> conv0+LN+GELU: Y [C][T][512], T = (n-10)/5+1 */
int artalk_op_w2v_front(const float* audio, int C, int n, const float* w, const float* bias, const float* lnw,
                        const float* lnb, float* xnorm_out, float* Y, void* stream);
/* audio front-end of inference.py:230-231: polyphase sinc FIR (torchaudio Resample defaults) + mean over channels.
 * x [nch][n] f32, taps [nw][2*width+orig] f32 (host-built, see artalk_amd/audio.py), out [n_out], the first n_out of
 * ceil(n*nw/orig) outputs.  ARTALK_EINVAL for a NULL pointer, nch, n, orig or nw <= 0, width < 0, n_out < 0, n_out > ceil(n*nw/orig)
 * (taken in 64 bits) or n_out > INT_MAX - 2^20; n_out == 0 launches nothing */
int artalk_op_resample_mean(const float* x, int nch, int n, const float* taps, int orig, int nw, int width, float* out, int n_out,
                            void* stream);
/* X [C][T][D] -> Y [C][181][D]: area pooling to {1,5,25,50,100} then SiLU */
int artalk_op_pool_silu(const float* X, int C, int T, int D, float* Y, void* stream);
/* ---- the same entry points with the site exponents of the P8 format and a status word (tests/test_p8_exps_ops_gpu.py) ----
 * Every P8 producer writes hi = f16(x * 2^e), lo = f16(x * 2^e - hi) and raises bit 3 of *status_dev (device int, may be NULL: no guard)
 * when |x| * 2^e > 65504 or x is NaN; every consumer removes the 2^e of the buffer it reads.  The entry points above call these with
 * e = 4 and no status word.  Any exponent outside [-8, 4] (what artalk_set_site_scales accepts): ARTALK_EINVAL before the device is touched.
 *   pack_split_ex        p8_exp: exponent of the packed activation (ignored for weights, which have no guard either)
 *   layernorm_ex         p8_exp: exponent of a P8 result (act | 0x100; D = 128 has no P8 form: ARTALK_EINVAL); rows r with
 *                        r % junk_period >= junk_from (junk_period > 0) are layout padding: stored as zeros, exempt from the guard
 *   gemm_f16s_packed_ex  a_exp: exponent A was packed with, or is split with while staging (fp32 A: force_cfg < 2, guarded); c_exp: exponent
 *                        of a P8 result (act bit 8) and of c2_u32, an optional second copy of an fp32 result in P8, same pitch (N % 8 == 0,
 *                        LDS-DMA configurations only): written by the kernel's epilogue where the planner fuses it (20 / 23 / 24 without
 *                        split-K), by a split pass over the result otherwise - as the model does
 *   gemm_f16s_ex         a_exp: exponent the fp32 A rows are split with while staging (or packed with, force_cfg | 0x100)
 *   attention_ex         qkv_exp: exponent of P8 Q / K / V rows (l2norm bit 2); out_p8 != 0: O is written in P8 with o_exp
 *   w2v_front_ex, pool_silu_ex   out_p8 != 0: Y is written in P8 with p8_exp (pool: D % 8 == 0)
 *   posconv_p8_ex        the grouped positional convolution of f16x3 mode (16 groups of 64 channels, 128 taps, padding 64): X
 *                        [n_chunks * Ts][1024] fp32, frames t < T of a chunk are read (split with a_exp while staged into LDS, guarded),
 *                        Wp [1024][128 * 64] packed weights with k = tap * 64 + input channel, C = R + act(conv + bias) for the rows
 *                        t < Ts <= 256 of every chunk (R may be NULL or C); pointers 16-byte aligned */
int artalk_op_pack_split_ex(const float* in, void* out_u32, int64_t n, int is_weight, int p8_exp, int* status_dev, void* stream);
int artalk_op_layernorm_ex(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift,
                           int M, int D, float eps, int act, int p8_exp, int junk_period, int junk_from, int* status_dev, void* stream);
int artalk_op_gemm_f16s_packed_ex(const void* A, int a_packed, int64_t lda, const void* Wp, const float* bias, float* C, int M, int N,
                                  int K, int act, int force_cfg, int a_exp, int c_exp, void* c2_u32, int* status_dev, void* stream);
int artalk_op_gemm_f16s_ex(const float* A, int64_t lda, const float* W, const float* bias, float* C, int M, int N, int K, int act,
                           int force_cfg, int a_exp, int* status_dev, void* stream);
int artalk_op_attention_ex(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                           float scale, int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8,
                           int* status_dev, void* stream);
int artalk_op_w2v_front_ex(const float* audio, int C, int n, const float* w, const float* bias, const float* lnw,
                           const float* lnb, float* xnorm_out, float* Y, int out_p8, int p8_exp, int* status_dev, void* stream);
int artalk_op_pool_silu_ex(const float* X, int C, int T, int D, float* Y, int out_p8, int p8_exp, int* status_dev, void* stream);
int artalk_op_posconv_p8_ex(const float* X, const void* Wp, const float* bias, const float* R, float* C, int n_chunks, int T, int Ts,
                            int act, int a_exp, int* status_dev, void* stream);
/* enc_out [B][100][32] -> hist_bits [B][181][32] u8, prev_fdec [B][100][32], msfeat [B][180][32] */
int artalk_op_bsq_history(const float* enc_out, uint8_t* hist_bits, float* prev_fdec, float* msfeat, int B, void* stream);
/* the same with the status word: bit 1 of *status_dev (device int, may be NULL) is raised when an element of enc_out is NaN/Inf */
int artalk_op_bsq_history_ex(const float* enc_out, uint8_t* hist_bits, float* prev_fdec, float* msfeat, int B, int* status_dev,
                             void* stream);
/* ---- the small kernels between the GEMMs of the AR / VAE / style stages, one launch each (tests/test_glue_ops_gpu.py) ----
 * Device pointers; sizes are the model's: 181 tokens of 32 bits per clip at levels of 1, 5, 25, 50, 100 tokens, embedding width 768,
 * 106 motion dims padded to 128 columns, 50 style frames.  NULL required pointers, B <= 0, n <= 0 and the cases named below:
 * ARTALK_EINVAL before the device is touched. */
/* logits [B * pn[level]][64] -> bits[b][off[level] + i][c] = logit pair c of token i has l1 > l0 (a tie gives 0); level < 4: fhat [B][100][32]
 * += the level's +-1/sqrt(32) upsampled to 100 frames, nextfeat [B][pn[level + 1]][32] = fhat area-pooled; level 4 leaves both alone (they
 * may be NULL).  Bit 0 of *status_dev (may be NULL) is raised for a NaN/Inf logit.  level outside 0..4: ARTALK_EINVAL. */
int artalk_op_ar_bits_next(const float* logits, uint8_t* bits, float* fhat, float* nextfeat, int B, int level, int* status_dev,
                           void* stream);
/* X[b * xrows + xoff + i][:] = We [768][32] . feat[b][i][:] + be + pos[i][:] for i < n; with style_cond: X[b * xrows][:] = style_cond[b] + pos0
 * (then xoff >= 1).  xrows >= xoff + n; We 16-byte aligned. */
int artalk_op_vq_embed(const float* feat, int n, const float* We, const float* be, const float* pos, float* X, int xrows, int xoff,
                       const float* style_cond, const float* pos0, int B, void* stream);
/* x0[b][:768] = style_cond[b] + lvlpos[:768]; fhat [B][100][32] = 0 */
int artalk_op_ar_begin(const float* style_cond, const float* lvlpos, float* x0, float* fhat, int B, void* stream);
/* X [B][200][32]: rows t < 100 = prev_fdec[b][t] + dpos[t]; rows 100 + t = fhat[b][t] + (+-1/sqrt(32) of bits[b][81 + t]) + dpos[100 + t] */
int artalk_op_dec_input(const float* prev_fdec, const float* fhat, const uint8_t* bits, const float* dpos, float* X, int B, void* stream);
/* m = dec[b][100 + t][:106] * std + mean -> out[b * out_bstride + (chunk * 100 + t) * 106 ..]; E [B][100][128] = (m - mean) / std + epos[t], columns
 * >= 106 zero.  Rows t < 100 of dec are not read.  Bit 2 of *status_dev (may be NULL) for a NaN/Inf m.  out_bstride (floats) must hold
 * chunk + 1 chunks. */
int artalk_op_dec_finish(const float* dec, const float* mean, const float* std_, const float* epos, float* out, int64_t out_bstride,
                         int chunk, float* E, int B, int* status_dev, void* stream);
/* E [B][100][128] = (0 - mean) / std + epos[t], columns >= 106 zero: the re-encoder input of the all-zero initial motion */
int artalk_op_enc_input_zero(const float* mean, const float* std_, const float* epos, float* E, int B, void* stream);
/* X [B * 50][128] = (motion [B * 50][106] - mean) / std, columns >= 106 zero */
int artalk_op_style_input(const float* motion, const float* mean, const float* std_, float* X, int B, void* stream);
/* X [M][D] += v [D] on every row */
int artalk_op_add_row(float* X, const float* v, int M, int D, void* stream);
/* style_cond [B][768]: has_style[b] == 1: 1.1 * (Ws [768][128] . mean over the 50 frames of feat [B * 50][128] + bs) - 0.1 * null_cond; == 2: a copy of
 * cached[b * cached_stride ..] (cached_stride >= 768 floats); else, or with has_style NULL: null_cond */
int artalk_op_style_finish(const float* feat, const float* Ws, const float* bs, const float* null_cond, const uint8_t* has_style,
                           float* style_cond, int B, const float* cached, int64_t cached_stride, void* stream);
/* dst[b * bytes ..] = src[0 .. bytes) for b < B; bytes % 16 == 0 and both pointers 16-byte aligned, else ARTALK_EINVAL */
int artalk_op_broadcast16(const void* src, void* dst, int64_t bytes, int B, void* stream);
/* Session pool moves.  A slot is [style | prev_in | prev_fdec] of s16 + p16 + f16 16-byte units; slots_dev: device table of n slot pointers.
 * gather: slot slots_dev[i] -> row i of the three buffers (rows of s16, p16, f16 units); scatter: the way back, the style field only
 * with with_style != 0.  All pointers 16-byte aligned, unit counts > 0. */
int artalk_op_session_gather(const float* const* slots_dev, float* style, float* prev_in, float* prev_fdec, int s16, int p16, int f16, int n,
                             void* stream);
int artalk_op_session_scatter(float* const* slots_dev, const float* style, const float* prev_in, const float* prev_fdec, int s16, int p16,
                              int f16, int n, int with_style, void* stream);
/* savgol_stream_kernel alone (artalk_session_smooth without a model): slots_dev is a device table of n pool slots in the library's layout
 * (the carry 142 976 floats behind the slot's start); seen, n_frames, last are host arrays [n]; raw [n][raw_stride], out [n][out_stride].
 * The per-row and stride checks of artalk_session_smooth run before the device is touched (ARTALK_EINVAL); artalk_op_rows_dry_run is
 * honoured; the stream is synchronised. */
int artalk_op_savgol_stream(float* const* slots_dev, const float* raw, int64_t raw_stride, const int* seen, const int* n_frames,
                            const uint8_t* last, float* out, int64_t out_stride, int n, void* stream);
/* every check of artalk_session_smooth on a session table made up by the caller - open ids with their frame counts and finished flags, ids a
 * scale change closed - and no device: returns what artalk_session_smooth would return before it enqueues anything, its message in msg,
 * and on ARTALK_OK the spans in first_out / count_out (optional) */
int artalk_op_session_smooth_check(const int64_t* open_ids, const int64_t* open_seen, const uint8_t* open_done, int n_open,
                                   const int64_t* ended_ids, int n_ended, const int64_t* ids, int n, int have_raw, int64_t raw_stride,
                                   const int* n_frames, const uint8_t* last, int64_t out_stride, int* first_out, int* count_out, char* msg,
                                   int msg_len);
/* *slot_dev = max(*slot_dev, bit pattern of max |x|) over rows x cols of an fp32 buffer of row pitch ld floats, or (is_p8) of the hi halves
 * of a P8 buffer times 2^-p8_exp; a NaN counts as +inf; rows r with r % junk_period >= junk_from (junk_period > 0) are skipped; rows == 0
 * changes nothing.  cols % 8 != 0, ld < cols or p8_exp outside [-8, 4]: ARTALK_EINVAL.  What artalk_calibrate reads its maxima with. */
int artalk_op_absmax(const float* buf, int rows, int cols, int64_t ld, int is_p8, int p8_exp, int junk_period, int junk_from,
                     unsigned int* slot_dev, void* stream);
/* ---- the GEMM, LayerNorm and attention launchers in the forms the AR / VAE / style bodies use them: row maps, pitches wider than a row,
 * column groups, batch strides, split-K finished by the plain or the LayerNorm-fused reduce (tests/test_rows_ops_gpu.py, tests/test_rows_ops_cpu.py) ----
 * A row map is int32 {rpb, bstride, off}: row(m) = (m / rpb) * bstride + off + m % rpb; rpb = INT32_MAX is the identity; rpb <= 0,
 * bstride < 0 or off < 0: ARTALK_EINVAL.  Every buffer that is addressed through a pitch, a map, a group stride or a batch stride comes
 * with its size in 4-byte elements counted from the pointer given; the entry point works out the furthest element the launch would touch
 * and returns ARTALK_EINVAL when it lies outside, as for every other bad argument (NULL required pointer, K % 32 != 0, an exponent outside
 * [-8, 4], a pointer or pitch the kernels' 16-byte accesses cannot take), before the device is touched.  All three synchronise the stream. */
/* C[cmap(m), n] = R[cmap(m), n] + gate[gmap(m), n] * act(sum_k A[m, k] W[n, k] + bias[n]), then optionally
 * Y[m, :] = LN(C[cmap(m), :]) * (1 + ln_scale[ln_mmap(m), :]) + ln_shift[ln_mmap(m), :] (N = 768, fp32 C): the order of the engine's gemm()
 * and its callers.
 *   mode       0: fp32 MFMA kernels (launch_gemm); 1: f16x3 LDS-DMA kernels with A already in P8 at a_exp (plan_gemm_p8 / launch_gemm_p8);
 *              2: bf16 kernels (launch_gemm_bf16).  W is fp32 [N][ldw]; the packed / bf16 copy is made internally.  Mode 1 needs every
 *              pointer 16-byte aligned, lda, ldw % 8 == 0 and N, ldc, ldr, ldg % 4 == 0 (the 16-byte epilogue); modes 0 and 2 need that of
 *              A, W, lda and ldw (% 4; mode 2: ldw % 8) only.
 *   force_cfg  -1 or 99: the launcher's / planner's own choice; mode 0: 1, 2, 3, 4 (artalk_op_gemm_ex); mode 1: 7, 8, 12, 20, 23, 24, 28, 31
 *              (artalk_op_gemm_f16s_packed); mode 2: 0, 1, 2 (artalk_op_gemm_bf16).
 *   splitk     1: none; S > 1 (S <= 16, 32 S <= K): S slabs in a temporary, finished by the reduce pass (mode 1: small-grid
 *              configurations only); 0: mode 1 with force_cfg -1 / 99: the planner's own split; otherwise none.
 *   ngrp       mode 1, column groups of the persistent 128x128 kernel (configuration 8): group j = columns [j ngrp, (j + 1) ngrp) reads weight
 *              rows at W + j grpW and bias at bias + j grpB and writes C + j grpC.  Taken with force_cfg 8, or with -1 / 99 where
 *              gemm_p8_eligible holds; no gate, residual, split-K or LayerNorm; otherwise ARTALK_EINVAL.
 *   ln_Y       non-NULL: the LayerNorm that follows, D = 768, no affine, Y dense rows of pitch ln_ldy, fp32 or (ln_out_p8) P8 at ln_p8_exp;
 *              ln_mod_elems counts from the lower of ln_scale and ln_shift.  With a split the reduce is launch_splitk_reduce_ln where
 *              splitk_reduce_ln_eligible holds (S in 2, 3, 4, 6, 8, every pointer 16-byte aligned and ln_ldy % 8 == 0 - also for an fp32 Y,
 *              for which the entry point itself takes ln_ldy % 4 == 0: such a pitch runs unfused and fused_ln says so), otherwise the
 *              plain reduce (or no reduce) and launch_layernorm, which reads C as dense rows: a cmap other than the identity is then
 *              ARTALK_EINVAL.  Y must not overlap C.
 *   R          may be C with ldr == ldc (the residual in place); any other overlap of R and C is ARTALK_EINVAL.
 *   used_cfg, used_splitk, fused_ln   host, nullable: the configuration and split that ran, whether the fused reduce did (0 / 1).
 *   cus        mode 1: the compute units of a CU partition (what a model under artalk_set_cu_mask passes to its GEMMs), 0 = the whole
 *              device.  It sizes the grid of the persistent kernels only - 7 / 12 run one workgroup per unit, 8 two - after rounding
 *              down to a multiple of 8 and clamping to [8, the device's count]; every other configuration ignores it.  The stream is
 *              NOT restricted to those units: the field changes which workgroup computes a tile, never a tile's arithmetic.
 *              cus < 0, or cus != 0 in modes 0 and 2: ARTALK_EINVAL. */
typedef struct artalk_op_gemm_rows_args {
    int32_t mode, M, N, K, act;
    const void* A; int64_t lda, a_elems; int32_t a_exp;
    const float* W; int64_t ldw, w_elems;
    const float* bias; int64_t bias_elems;
    void* C; int64_t ldc, c_elems; int32_t cmap[3];
    const float* gate; int64_t ldg, gate_elems; int32_t gmap[3];
    const float* R; int64_t ldr, r_elems;          /* addressed with cmap; may be C */
    int32_t c_p8, c_exp;
    int32_t force_cfg, splitk;
    int32_t ngrp; int64_t grpW, grpB, grpC;
    int32_t* status_dev;
    void* ln_Y; int64_t ln_ldy, ln_y_elems;
    const float* ln_scale; const float* ln_shift; int64_t ln_ldm, ln_mod_elems; int32_t ln_mmap[3];
    float ln_eps; int32_t ln_out_p8, ln_p8_exp;
    int32_t* used_cfg; int32_t* used_splitk; int32_t* fused_ln;
    int32_t cus;
} artalk_op_gemm_rows_args;
int artalk_op_gemm_rows(const artalk_op_gemm_rows_args* a, void* stream);
/* sizeof(artalk_op_gemm_rows_args) followed by the offset of every field in declaration order (50 values; returns the count, ARTALK_EINVAL
 * for n below it): what a binding checks its mirror of the struct against */
int artalk_op_gemm_rows_layout(int64_t* out, int n);
/* enable != 0: on the calling thread the three *_rows entry points validate as usual and return ARTALK_OK where they would first touch the
 * device (artalk_op_gemm_rows still reports used_cfg, used_splitk, fused_ln): what separates "accepted" from "refused" without a GPU */
int artalk_op_rows_dry_run(int enable);
/* artalk_op_layernorm_ex with row pitches ldx, ldy >= D, the modulation rows at scale / shift + mmap(m) * ldm (ldm >= D; mod_elems counts
 * from the lower of the two pointers) and the sizes of X, Y and the modulation table.  Y may be X with ldy == ldx; any other overlap is
 * ARTALK_EINVAL */
int artalk_op_layernorm_rows(const float* X, float* Y, const float* w, const float* b, const float* scale, const float* shift, int M,
                             int D, float eps, int act, int p8_exp, int junk_period, int junk_from, int* status_dev, int64_t ldx,
                             int64_t ldy, int64_t ldm, const int32_t* mmap, int64_t x_elems, int64_t y_elems, int64_t mod_elems,
                             void* stream);
/* artalk_op_attention_ex with row pitches (>= H * HD), batch strides (>= 0; O's batches must not overlap) and buffer sizes: clip b, row i,
 * head h of Q is at Q + b * q_bstride + i * ldq + h * HD, likewise K, V (Lk rows) and O */
int artalk_op_attention_rows(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                             float scale, int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8,
                             int* status_dev, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bstride, int64_t k_bstride,
                             int64_t v_bstride, int64_t o_bstride, int64_t q_elems, int64_t k_elems, int64_t v_elems, int64_t o_elems,
                             void* stream);
/* The kernels of attention.hip, one value per instantiation: what artalk_op_attention_plan returns and artalk_op_attention_rows_cus reports */
#define ARTALK_ATTN_F32_64 0          /* attention_kernel<64>: fp32 MFMAs, 64-query workgroups */
#define ARTALK_ATTN_F32_32 1          /* attention_kernel<32> (the style encoder's 32-wide heads) */
#define ARTALK_ATTN_SHORT 2           /* attention_short_kernel: fp32, keys split over the waves (Lq <= 64, Lk >= 64, no mask) */
#define ARTALK_ATTN_F16 3             /* attention_f16_kernel<1>: f16-split MFMAs, fp32 rows, 64-query workgroups */
#define ARTALK_ATTN_F16_P8 4          /* attention_f16_kernel<1, 1>: the same on P8 rows */
#define ARTALK_ATTN_F16_WIDE 5        /* attention_f16_wide_kernel: P8 rows, one workgroup per head, all keys staged once */
#define ARTALK_ATTN_F16_PP 6          /* attention_f16_pp_kernel: P8 rows, persistent, two LDS buffers filled by LDS-DMA */
#define ARTALK_ATTN_F16_WIDE_AR 7     /* attention_f16_wide_ar_kernel<1>: fp32 rows, one 7-wave workgroup per head, 192 keys per phase */
#define ARTALK_ATTN_F16_WIDE_AR_P8 8  /* attention_f16_wide_ar_kernel<1, 1, 7, 128>: P8 rows, 7-wave workgroups of 112 queries, 128 keys per phase */
/* Which kernel an attention launch of this shape runs on a device of n_cu compute units (> 0), for a model partition of cus units
 * (0 = the whole device; >= 0): plan_attention, the function launch_attention switches on, asked without a device.  l2norm is the flag
 * word of artalk_op_attention_ex (| 1 L2 norm, | 2 f16-split kernels, | 4 P8 rows), split its mask.  Returns ARTALK_ATTN_*, or
 * ARTALK_EINVAL for what artalk_op_attention_rows refuses in these arguments.  The environment switches ARTALK_ATTN_WIDE and
 * ARTALK_ATTN_PP (each read once per process) take part in the answer as they do in a launch. */
int artalk_op_attention_plan(int B, int H, int HD, int Lq, int Lk, int l2norm, int split, int cus, int n_cu);
/* artalk_op_attention_rows (which forwards here with cus = 0, used_kernel = NULL) for a model partition of cus compute units
 * (AttnArgs::cus: the grid and the heads-per-unit threshold of the persistent kernel; the stream is NOT restricted to them; cus < 0:
 * ARTALK_EINVAL).  used_kernel (host, nullable) receives the ARTALK_ATTN_* value that ran; under artalk_op_rows_dry_run, the plan for
 * a device of 256 units. */
int artalk_op_attention_rows_cus(const float* Q, const float* K, const float* V, float* O, int B, int H, int HD, int Lq, int Lk,
                                 float scale, int l2norm, const float* qscale, int split, int qkv_exp, int o_exp, int out_p8,
                                 int* status_dev, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_bstride, int64_t k_bstride,
                                 int64_t v_bstride, int64_t o_bstride, int64_t q_elems, int64_t k_elems, int64_t v_elems, int64_t o_elems,
                                 int cus, int* used_kernel, void* stream);
/* ---- the wav2vec2 stage's kernels in the chunk-strided forms run_wav2vec launches them (tests/test_w2v_ops_gpu.py, tests/test_w2v_ops_cpu.py).
 * Conventions of the *_rows entry points above: every buffer reached through an offset, a pitch or a stride comes with its size in 4-byte
 * elements, the furthest element of the launch is worked out on the host, any bad argument is ARTALK_EINVAL before the device is touched,
 * artalk_op_rows_dry_run is honoured, the stream is synchronised.  (The conv layers 1-6 are artalk_op_gemm_rows with lda < K, the encoder
 * attention is artalk_op_attention_rows with its strides: they need no entry point of their own.) */
/* artalk_op_w2v_front_ex with the chunk table and the row stride of the model: chunk c is read at audio + chunk_off[c] (host table of C
 * offsets in samples; they may overlap and come in any order) and frame t < T = (n - 10) / 5 + 1 of chunk c is written to row
 * c * row_stride + t of Y (512 wide); rows t >= T of a chunk are not written.  xnorm_out stays [C][n].  ARTALK_EINVAL: a NULL pointer, a negative
 * offset, chunk_off[c] + n > audio_elems, row_stride < T, a Y too small or not 16-byte (out_p8: 32-byte) aligned, p8_exp outside [-8, 4]. */
int artalk_op_w2v_front_rows(const float* audio, int64_t audio_elems, const int64_t* chunk_off, int C, int n, const float* w,
                             const float* bias, const float* lnw, const float* lnb, float* xnorm_out, float* Y, int64_t row_stride,
                             int64_t y_elems, int out_p8, int p8_exp, int* status_dev, void* stream);
/* artalk_op_pool_silu_ex with the frame stride of the model: frame t < T of chunk c is read at row c * x_tstride + t of X (D wide, D % 4 == 0;
 * out_p8: D % 8 == 0), x_tstride >= T >= 1; Y [C][181][D].  X 16-byte, Y 16-byte (out_p8: 32-byte) aligned. */
int artalk_op_pool_silu_rows(const float* X, int C, int T, int D, float* Y, int out_p8, int p8_exp, int* status_dev, int64_t x_tstride,
                             int64_t x_elems, int64_t y_elems, void* stream);
/* The grouped positional convolution as run_wav2vec sets it up: X [n_chunks * Ts][groups * cg] fp32, frames t < T of a chunk are read and
 * everything outside [0, T) of the chunk counts as zero (padding taps / 2, the last output frame dropped); W fp32 [groups * cg][taps * cg]
 * with k = tap * cg + input channel of the group (packed / converted internally); C = R + act(conv + bias) for the rows t < Ts of every
 * chunk, pitch groups * cg; R is NULL or C (the residual in place); X must not overlap C.
 *   mode 0: the fp32 grouped GEMM over grid.z (amode 1 of launch_gemm), force_cfg -1 or 1, 2, 3, 4;
 *   mode 1: launch_posconv_p8 (the window split with 2^a_exp while staged, guarded through status_dev): groups = 16, cg = 64, taps = 128,
 *           Ts <= 256, force_cfg -1, X, W, bias and C 16-byte aligned;
 *   mode 2: the bf16 grouped GEMM (amode 1 of launch_gemm_bf16), force_cfg -1 or 0, 1, 2.
 * Modes 0 and 2 take any cg % 4 == 0 with (cg * taps) % 32 == 0, X and W 16-byte aligned. */
int artalk_op_posconv_rows(int mode, const float* X, int64_t x_elems, const float* W, const float* bias, const float* R, float* C,
                           int64_t c_elems, int n_chunks, int T, int Ts, int groups, int cg, int taps, int act, int a_exp, int force_cfg,
                           int* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARTALK_HIP_H */
