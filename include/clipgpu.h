/*
 * clipgpu — MI355X-native CLIP embedding engine, C ABI.
 *
 * This is the drop-in boundary for the hot path of RuurdBijlsma/clip-embedder-rs
 * (crate open_clip_inference v0.4.0):
 *
 *     image/text -> preprocess/tokenize -> ViT / text transformer -> L2-normalised [B, E]
 *
 * Each entry point names the reference interface it replaces (file:line under the
 * reference tree).  Conventions mirror the reference:
 *   - caller owns every input/output buffer; the engine copies in and out
 *     (Value::from_array + .to_owned(), src/vision.rs:105-113, src/text.rs:153-166);
 *   - return 0 on success, non-zero on error; clipgpu_last_error() gives the
 *     thread-local message (maps to ClipError::Inference / ::Config / ::Io, src/error.rs:9-41);
 *   - an empty batch is an error "Empty batch" (src/vision.rs:121-123);
 *   - one call per handle at a time: each handle serialises its callers with an internal
 *     mutex (the reference's RwLock write lock, src/vision.rs:107, src/text.rs:155);
 *     separate handles are independent (duplicate(), src/vision.rs:86-91).
 * No torch / ndarray / ort types cross this boundary: plain pointers and sizes only.
 */
#ifndef CLIPGPU_H
#define CLIPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 4 with the embedding index section: that change only adds symbols; every existing entry
 * point keeps its signature, its behaviour and its bits. */
#define CLIPGPU_ABI_VERSION 4

enum clipgpu_status {
  CLIPGPU_OK = 0,
  CLIPGPU_ERR_INVALID = 1,   /* bad argument / shape          -> ClipError::Inference / Shape */
  CLIPGPU_ERR_CONFIG = 2,    /* model dir / config problem    -> ClipError::Config / MissingModelFile */
  CLIPGPU_ERR_IO = 3,        /* file system                   -> ClipError::Io */
  CLIPGPU_ERR_DEVICE = 4,    /* HIP / RCCL failure            -> ClipError::Inference */
  CLIPGPU_ERR_TOKENIZER = 5  /* tokenizer failure             -> ClipError::Tokenizer */
};

enum clipgpu_tower { CLIPGPU_TOWER_VISION = 0, CLIPGPU_TOWER_TEXT = 1 };
/* CLIPGPU_DTYPE_FP8: the fp8 weight path of BASELINE configs[4] -- the QKV, c_fc and c_proj
 * GEMMs run as MX-fp8 (OCP e4m3 weights and activations, E8M0 scale per 32 K-elements,
 * block-scaled MFMA); attention, out_proj, stems and heads run in bf16.  Needs width and MLP
 * width % 128 == 0.  Lossy: the embeddings do not meet the bf16 path's cosine bar. */
enum clipgpu_dtype { CLIPGPU_DTYPE_BF16 = 0, CLIPGPU_DTYPE_F16 = 1, CLIPGPU_DTYPE_FP8 = 2 };

typedef struct clipgpu_engine clipgpu_engine;       /* one tower on one or more GPUs (== one OnnxSession) */
typedef struct clipgpu_tokenizer clipgpu_tokenizer; /* CLIP BPE tokenizer (== tokenizers::Tokenizer) */

/* Thread-local message for the last failed call on this thread ("" if none). */
const char* clipgpu_last_error(void);
int clipgpu_abi_version(void);
/* sha256 fingerprint of the sources this library was built from (binary provenance; the
 * Python host refuses a library whose fingerprint differs from its tree's). */
const char* clipgpu_build_source_hash(void);

/* ---- engine lifecycle ----------------------------------------------------------------
 * Replaces OnnxSession::new (src/onnx.rs:13-30) as called by VisionEmbedder::from_local_dir
 * (src/vision.rs:58-84) / TextEmbedder::from_local_dir (src/text.rs:54-101).
 * model_dir must hold open_clip_config.json and model_config.json plus a weight source, in
 * this order of preference: open_clip_model.safetensors; the reference's own export
 * visual.onnx / text.onnx (+ .onnx.data external data, pull_onnx.py:170-195; initializers by
 * open_clip name, with or without the "model." wrapper prefix); or clipgpu_synthetic.json
 * {"seed": N} (seeded weights).
 * device_ids/n_devices: the GPUs this handle replicates the weights onto (data-parallel
 * batch sharding across them); NULL/0 = device 0.  max_batch: rows per device per launch
 * (larger batches are processed in chunks).
 * Speed (never the output bits): the GEMM tiles and lane count come from a table measured on
 * MI355X (engine/tiles.hip table_tiles / table_lanes) for one lane's token rows at max_batch: the
 * measured regimes are >= 2048 rows per lane (ViT-B/32 vision 256, text 1024, SO400M 128, H/14
 * 64 per GPU); smaller max_batch uses the shape heuristic (skinny kernel at <= 256 rows), and
 * clipgpu_options.tuning = 1 times the candidates at creation for any other batch. */
int clipgpu_create(const char* model_dir, int tower, const int* device_ids, int n_devices, int dtype,
                   int max_batch, clipgpu_engine** out);
void clipgpu_destroy(clipgpu_engine* e);

/* Per-engine options (clipgpu_create_ex; clipgpu_create == clipgpu_create_ex with opts = NULL).
 * The reference builds each tower's session with its own SessionBuilder settings
 * (src/onnx.rs:13-30); these are this engine's equivalents, per handle, so one process can hold
 * e.g. an fp8 vision tower beside a bf16 text tower with different MX splits. */
#define CLIPGPU_MX_QKV 1u  /* fp8 engines: the QKV projection runs as an MX-fp8 GEMM */
#define CLIPGPU_MX_FC 2u   /* c_fc */
#define CLIPGPU_MX_PROJ 4u /* c_proj (needs CLIPGPU_MX_FC: c_fc's epilogue quantizes the hidden rows) */
#define CLIPGPU_RESIDUAL_F32 1
#define CLIPGPU_RESIDUAL_F16 2
typedef struct clipgpu_options {
  uint32_t struct_size; /* sizeof(clipgpu_options) (set by clipgpu_options_init); an older caller's
                           smaller struct keeps the defaults of the fields it does not have */
  uint32_t mx_sites;    /* fp8 engines: CLIPGPU_MX_* bits; 0 = default (all three) */
  int32_t lanes;        /* concurrent sub-batch lanes per device, 1..4; 0 = the tile table's choice */
  int32_t tuning;       /* 0 = GEMM tiles and lanes from the committed MI355X tile table
                           (deterministic, default); 1 = time the candidates at creation, per site and
                           then over whole forwards; 2 = the per-site timing only (the choice then
                           depends on the timings; it never changes the output bits) */
  int32_t communicator; /* handles over > 1 distinct devices: 1 = create the RCCL communicator at
                           creation; 0 (default) = on the first gathered call */
  /* ---- ABI v3 (round 4): every engine behaviour is a field here; the library reads no
   * environment variables.  0 is the default everywhere. */
  int32_t graphs;       /* 0 / 1 = replay each forward as a captured hipGraph (default); -1 = launch
                           the kernels directly (bit-identical) */
  int32_t prune_last;   /* 0 / 1 = the last layer runs on the pooled rows only (default; bit-identical);
                           -1 = on every token */
  int32_t trim_text;    /* 0 / 1 = host-id text batches run on their first max(EOT index) + 1 tokens
                           (default; bit-identical); -1 = on the full context */
  int32_t gemm_tiles[4]; /* GEMM tile per trunk site (qkv, out_proj, c_fc, c_proj): 0 = the table's
                           (or tuner's) choice, -1 = the shape heuristic, else a GemmTile id the library
                           builds (csrc/kernels/kernels.hpp kGemmTiles; speed only, never the bits) */
  int32_t patch_tile;   /* the vision patch-embedding GEMM's tile, as gemm_tiles */
  uint32_t mx_layers;   /* fp8 engines: bit l set = layer l runs its MX sites in MX-fp8, the other layers
                           run every GEMM in bf16; 0 = every layer (default).  Layers 0..31 only (a
                           tower's layers >= 32 run bf16 under a non-zero mask); a bit at or beyond the
                           tower's layer count is refused (CLIPGPU_ERR_INVALID) */
  /* ---- ABI v4 (round 5) */
  int32_t residual;     /* storage of the residual stream x: 1 = f32; 2 = f16 (half the bytes of x's two
                           read-modify-writes and two LayerNorm reads per layer; every add into x and every
                           LayerNorm statistic stays f32; CLIP-family engines of every dtype, SigLIP
                           CLIPGPU_ERR_INVALID); 0 = the default: f16 where it applies, else f32.  f16 holds
                           |x| <= 65504 (a larger value is stored as inf); CLIP / DFN residual streams stay in
                           the hundreds (tests/test_gpu_parity.py test_massive_residual_channels_parity):
                           choose 1 for a checkpoint whose stream exceeds that range */
  int32_t ln_fold;      /* ln_1 / ln_2 folded into the QKV / c_fc GEMMs (f16 residual stream only): the GEMM
                           reads x itself with W' = W diag(gamma) in f16 and applies each row's mean / rstd
                           and bias + W beta in its epilogue; the rows' (mean, rstd) come from a statistics-only
                           pass (8 bytes per row) instead of a normalised copy of x.  0 = the default: on where
                           it applies (bf16 / f16 engines, residual f16, QuickGELU / GELU MLP); 1 = on
                           (CLIPGPU_ERR_INVALID where it does not apply); -1 = off (LayerNorm kernels + bf16 /
                           f16 GEMMs) */
} clipgpu_options;
/* Fills *opts with the defaults. */
int clipgpu_options_init(clipgpu_options* opts);
int clipgpu_create_ex(const char* model_dir, int tower, const int* device_ids, int n_devices, int dtype,
                      int max_batch, const clipgpu_options* opts, clipgpu_engine** out);
/* The engine's resolved choices: tiles[4] = GemmTile per trunk site (qkv, out_proj, c_fc, c_proj),
 * *lanes = concurrent lanes of a device-side forward, *mx_sites = CLIPGPU_MX_* bits in use. */
int clipgpu_engine_info(const clipgpu_engine* e, int tiles[4], int* lanes, uint32_t* mx_sites);

int clipgpu_embed_dim(const clipgpu_engine* e);      /* E */
int clipgpu_input_size(const clipgpu_engine* e);     /* vision: image_size S; text: context length T */
int clipgpu_num_devices(const clipgpu_engine* e);

/* ---- vision forward ------------------------------------------------------------------
 * Replaces session.run(pixel_values) + extract in VisionEmbedder::embed_images
 * (src/vision.rs:100-117).  nchw: [B,3,S,S] f32, already normalised (preprocess_batch
 * output, src/vision.rs:119-135).  out: [B,E] f32 row-major, L2-normalised. */
int clipgpu_embed_pixels(clipgpu_engine* e, const float* nchw, int64_t B, int64_t S, float* out);

/* Device-side-normalise variant: nhwc u8 [B,S,S,3] (already resized/cropped), mean/std
 * applied on the GPU exactly as normalize_pixels (src/vision.rs:235-259). */
int clipgpu_embed_u8(clipgpu_engine* e, const uint8_t* nhwc, int64_t B, int64_t S, const float mean[3],
                     const float std[3], float* out);

/* ---- caller-registered host buffers ------------------------------------------------------
 * The reference's embed_images / embed_texts hand host arrays to the session (src/vision.rs:102-113,
 * src/text.rs:150-166).  By default the host-buffer entry points stage them through the handle's
 * pinned buffers (a host copy, then the PCIe DMA).  A caller that reuses its buffers can pin them once
 * (hipHostRegister, mapped and portable): an embed_* call whose whole input (or output) lies inside a
 * registered range then DMAs straight from (into) it, skipping the host copy; the batch still moves
 * in one chunk per lane, so the first chunk's transfer is what is exposed before the forward starts.
 * Results are bit-identical either way.  Process-wide; the caller keeps the memory alive, and
 * unregisters it only when no embed_* call is using it, before freeing it.  Ranges may not overlap. */
int clipgpu_host_register(void* ptr, size_t bytes);
int clipgpu_host_unregister(void* ptr);

/* ---- text forward ---------------------------------------------------------------------
 * Replaces session.run(input_ids [, attention_mask]) in TextEmbedder::embed_texts
 * (src/text.rs:148-169).  ids: [B,T] int64; mask may be NULL (the exported text graph has
 * no mask input, pull_onnx.py:296-302; it is accepted and ignored, as the reference does
 * when the graph lacks "attention_mask", src/text.rs:156-161).  The batch runs on its first
 * max(EOT index)+1 tokens (at least 16; bit-identical to the full context under causal
 * attention and argmax pooling; clipgpu_options.trim_text = -1 disables). */
int clipgpu_embed_tokens(clipgpu_engine* e, const int64_t* ids, const int64_t* mask, int64_t B, int64_t T,
                         float* out);

/* ---- device-resident entry points (benchmarks, zero-copy pipelines) ----------------------
 * Inputs/outputs are device pointers on the handle's first device; work is ordered on
 * `stream` (a hipStream_t; NULL = the legacy default stream, as in HIP's own APIs, which is
 * also torch's default stream) and the call returns without synchronising: work enqueued on
 * `stream` before the call is complete before the forward reads its input, and work enqueued
 * after it sees the finished embeddings.  The forward itself runs as a hipGraph on the
 * handle's stream, forked from and joined back to `stream` by events.  B <= max_batch. */
int clipgpu_embed_pixels_device(clipgpu_engine* e, const float* d_nchw, int64_t B, float* d_out, void* stream);
int clipgpu_embed_u8_device(clipgpu_engine* e, const uint8_t* d_nhwc, int64_t B, const float mean[3],
                            const float std[3], float* d_out, void* stream);
int clipgpu_embed_tokens_device(clipgpu_engine* e, const int64_t* d_ids, int64_t B, float* d_out, void* stream);

/* Decoded images straight to embeddings, crop/resize on the GPU (a3-a7 on the device).
 * Replaces preprocess_batch + session.run in VisionEmbedder::embed_images
 * (src/vision.rs:100-162): images[i] is [heights[i]][widths[i]][3] u8 (DynamicImage::to_rgb8
 * layout, any size); the model folder's preprocess_cfg (interpolation, resize_mode, mean,
 * std; src/config.rs:49-64) applies.  The GPU resize uses the host resize's fixed-point
 * tables, so results are bit-identical to clipgpu_preprocess_batch + clipgpu_embed_pixels.
 * out: [n,E] f32, L2-normalised. */
int clipgpu_embed_images_rgb8(clipgpu_engine* e, const uint8_t* const* images, const int* widths, const int* heights,
                              int64_t n, float* out);

/* ---- host preprocessing (src/vision.rs:119-259) ----------------------------------------
 * rgb: [h][w][3] u8 (DynamicImage::to_rgb8 layout).  Resize with the crop box of
 * resize_with_fast_image_resize (src/vision.rs:164-198): unless resize_mode == "squash",
 * the centred min(w,h) square; interpolation "bicubic" (CatmullRom) / "bilinear" / other
 * (nearest).  Then normalize_pixels (src/vision.rs:235-259) into out_chw [3][size][size]. */
int clipgpu_preprocess_rgb8(const uint8_t* rgb, int width, int height, int size, const char* interpolation,
                            const char* resize_mode, const float mean[3], const float std[3], float* out_chw);
/* Resize/crop only: out_rgb [size][size][3] u8. */
int clipgpu_resize_rgb8(const uint8_t* rgb, int width, int height, int size, const char* interpolation,
                        const char* resize_mode, uint8_t* out_rgb);
/* Batch preprocess with a host thread pool (preprocess_batch's rayon loop, src/vision.rs:128-132):
 * images[i] is [heights[i]][widths[i]][3] u8; out: [n][3][size][size]. */
int clipgpu_preprocess_batch(const uint8_t* const* images, const int* widths, const int* heights, int64_t n,
                             int size, const char* interpolation, const char* resize_mode, const float mean[3],
                             const float std[3], float* out);
/* The crate's non-default resize, resize_with_image (src/vision.rs:200-233; the build without the
 * `fast_image_resize` feature): the image crate 0.25.9's imageops::resize (f32 separable filter,
 * vertical pass then horizontal, CatmullRom / Triangle / Nearest) to round(W*s) x round(H*s),
 * s = size / min(W, H), then crop_imm at the rounded centre offsets ("squash": resize_exact to
 * size x size).  Same arguments and outputs as clipgpu_resize_rgb8 / clipgpu_preprocess_batch. */
int clipgpu_resize_rgb8_image(const uint8_t* rgb, int width, int height, int size, const char* interpolation,
                              const char* resize_mode, uint8_t* out_rgb);
int clipgpu_preprocess_batch_image(const uint8_t* const* images, const int* widths, const int* heights, int64_t n,
                                   int size, const char* interpolation, const char* resize_mode, const float mean[3],
                                   const float std[3], float* out);

/* ---- tokenizer (src/text.rs:62-139) ----------------------------------------------------
 * Loads a HF tokenizers CLIP tokenizer.json (BPE + ByteLevel, </w> suffix) and applies
 * with_padding(Fixed(context_length), pad_id) + with_truncation(max_length=context_length)
 * as TextEmbedder::from_local_dir does (src/text.rs:70-85).  pad_id < 0: look up "<pad>"
 * in the vocab (src/text.rs:70-73). */
int clipgpu_tokenizer_create(const char* tokenizer_json, int context_length, int64_t pad_id,
                             clipgpu_tokenizer** out);
void clipgpu_tokenizer_destroy(clipgpu_tokenizer* t);
/* texts: n UTF-8 strings; lengths[i] = byte length of texts[i] (like a Rust &str, may contain NUL),
 * or lengths == NULL for NUL-terminated strings.  lowercase != 0 applies str::to_lowercase first
 * (tokenizer_needs_lowercase, src/text.rs:115-117).  ids, mask: [n][context_length]. */
int clipgpu_tokenize(clipgpu_tokenizer* t, const char* const* texts, const int64_t* lengths, int64_t n,
                     int lowercase, int64_t* ids, int64_t* mask);
/* Token id of a vocab string, or -1. */
int64_t clipgpu_tokenizer_token_id(const clipgpu_tokenizer* t, const char* token);
int64_t clipgpu_tokenizer_vocab_size(const clipgpu_tokenizer* t);

/* ---- Clip facade math for many images x many labels -------------------
 * The src/clip.rs:79-185 arithmetic on the GPU: logits[i][j] = dot(img[i], txt[j]).mul_add(
 * logit_scale, logit_bias) (ModelConfig defaults 1.0 / 0.0 are the caller's), then
 *   activation CLIPGPU_SIM_SOFTMAX: max-subtracted softmax along `axis` -- 1 = over the labels
 *     of each image (classify, :92-132), 0 = over the images of each label (rank_images,
 *     :134-170);  CLIPGPU_SIM_SIGMOID: elementwise sigmoid (activation_function "sigmoid");
 *   CLIPGPU_SIM_LOGITS: the logits themselves (compare, :79-90).
 * img [n_img][E], txt [n_txt][E] f32 (the embed_* outputs); out [n_img][n_txt] f32; E % 16 == 0,
 * n_img <= 65535 * 64 = 4194240, n_txt <= 2^30, n_img * n_txt <= 2^40 (anything else: CLIPGPU_ERR_INVALID,
 * "Shape error: ...").
 * Host-buffer form on GPU `device`; the _device form takes device pointers and a stream.
 * (The descending sort of classify / rank_images stays on the host.) */
enum clipgpu_sim_activation { CLIPGPU_SIM_SOFTMAX = 0, CLIPGPU_SIM_SIGMOID = 1, CLIPGPU_SIM_LOGITS = 2 };
int clipgpu_similarity(int device, const float* img, int64_t n_img, const float* txt, int64_t n_txt, int64_t E,
                       float logit_scale, float logit_bias, int activation, int axis, float* out);
int clipgpu_similarity_device(const float* d_img, int64_t n_img, const float* d_txt, int64_t n_txt, int64_t E,
                              float logit_scale, float logit_bias, int activation, int axis, float* d_out,
                              void* stream);

/* ---- embedding index: a device-resident gallery with fused top-k search ----------------------
 * What the reference's users do with the embeddings: store the image embeddings and "search with the
 * text embedding through images using cosine similarity" (README.md:76-82; examples/search.rs),
 * best first as Clip::rank_images returns them (src/clip.rs:134-170).  The gallery stays on GPU
 * `device` between calls (the *_device embed entry points can feed it without a host round trip);
 * a search returns only the k best rows per query, the [n_q][N] score matrix never exists.
 *   score(i, j) = dot(queries[i], gallery[j]).mul_add(logit_scale, logit_bias) -- bit-identical to
 *     clipgpu_similarity(..., CLIPGPU_SIM_LOGITS) on the same inputs (logits; the probabilities of
 *     Clip::rank_images / Clip::classify come from clipgpu_index_search_probs, below);
 *   order: descending score, equal scores by ascending gallery index (the reference's stable
 *     sort_by(partial_cmp), src/clip.rs:160-166); +0.0 == -0.0; a NaN score ranks below -inf
 *     (L2-normalised embeddings never produce one).
 * Rows are appended in call order and an index is a row's position in that order.  E % 16 == 0,
 * capacity < 2^31 rows, fixed at creation: the gallery, one search workspace (at most 64 MiB) and
 * the host forms' staging are allocated there and never reallocated; an add beyond the capacity is
 * CLIPGPU_ERR_INVALID "index full" and leaves the index unchanged.  1 <= k <= CLIPGPU_TOPK_MAX
 * (larger k: the whole matrix via clipgpu_similarity).  out_idx [nq][k] int64, out_score [nq][k] f32
 * (the logits' own bits); slots beyond min(k, size) hold index -1 and score -inf.  Any nq: queries
 * run in chunks sized to the workspace.  nq <= 0 or an empty index: "Empty batch".
 * A handle serialises its callers (mutex).  The _device forms take device pointers on `device`, are
 * ordered on `stream` (NULL = the legacy default stream) and return without synchronising; the
 * handle also orders each operation after its previous one by an event, so an add on one stream
 * followed by a search on another sees the added rows.  The host forms synchronise.
 *
 * Storage type (clipgpu_index_create_ex; clipgpu_index_create is CLIPGPU_INDEX_F32).  The memory
 * follows the row bytes: a million 512-d rows are 2 GiB in f32 and 1 GiB in f16 / bf16.  The time
 * does not yet: measured over 2^20 x 512 rows, one query takes 0.47 ms on f32 and 0.43 ms on f16 /
 * bf16 (about 8 % less, not half), 16 queries take the same on all three, and so do 17 and more:
 * the few-query kernel is bound by its staging through on-chip memory, not by reading the gallery,
 * and the wide kernel by its arithmetic (embedding index).  Choose a 16-bit type for
 * the memory.  add and add_device still take f32 rows (add_device: d_rows 16-byte aligned for a
 * 16-bit index, whose convert kernel reads them four at a time; an F32 index copies them and asks
 * only for f32 alignment); a 16-bit index rounds them on the device, round to nearest even: f16 keeps subnormals
 * (2^-24 .. 2^-14) and sends |x| >= 65520 to +-inf (65504 is the largest finite value); bf16 keeps
 * f32's exponent range; NaN stays NaN and -0.0 stays -0.0.  Queries stay f32 and the score is
 * unchanged, fmaf(dot(q, widen(row)), scale, bias) on the same k-ascending exact-f32 chain
 * (widening is exact): a 16-bit index returns exactly what an F32 index holding
 * widen(round(rows)) returns, bit for bit.  Against the F32 index of the unrounded rows a logit
 * moves by at most (derived, not measured)
 *   |dscore| <= |scale| * u * sum_i |q_i g_i| <= |scale| * u * ||q|| ||g||,
 *   u = 2^-11 (f16, normal range) or 2^-8 (bf16):
 * 0.049 (f16) and 0.39 (bf16) at scale 100 on unit rows; the two f32 chains' own rounding adds
 * about E * 2^-23 * sum_i |q_i g_i| on top.  clipgpu_index_get_rows copies rows [first, first + n)
 * as stored, widened to f32, to host memory [n][E] (ordered after the handle's last operation; it
 * synchronises): an export of the index, and the rounding made visible.  For a 16-bit index,
 * clipgpu_index_add and clipgpu_index_get_rows pass the f32 rows through a device scratch buffer
 * (at most 64 MiB) that the handle allocates at the first such call and keeps until it is destroyed.  first < 0, n <= 0 or
 * first + n > size is CLIPGPU_ERR_INVALID; an unknown dtype is CLIPGPU_ERR_INVALID "unknown index
 * dtype", raised like the other create-time errors before any device call.
 *
 * Few queries: a launch of at most 16 query rows (the last chunk of any call included) may run a
 * few-query kernel instead of the 64-row-tile one.  The results are bit-identical; the route shows
 * only in the time (embedding index, has the measured threshold).
 *
 * Removal, replacement and filters.  clipgpu_index_remove marks the rows at `ids` (host, n of them) dead:
 * a dead row never appears in a result, every other row keeps its position (a caller's ids are stable)
 * and clipgpu_index_size is unchanged -- it counts slots; clipgpu_index_live counts the live rows.
 * Removing a dead row is a no-op and ids may repeat; an id outside [0, size) is CLIPGPU_ERR_INVALID and
 * nothing changes.  clipgpu_index_get_live writes one byte per row of [first, first + n), 1 = live (the
 * range rules of clipgpu_index_get_rows).  clipgpu_index_set_rows overwrites the rows at `ids` with host
 * f32 rows [n][E] (a 16-bit index rounds them exactly as add does) and marks them live: the way to reuse
 * the slot of a removed row instead of running out of capacity.  Every id must be < size and none may
 * repeat, else CLIPGPU_ERR_INVALID and nothing changes.  add / add_device append live rows as before;
 * clipgpu_index_clear makes every future row live again.  remove, get_live and set_rows synchronise.
 *   clipgpu_index_search_filtered[_device] search the rows that are live AND allowed.  `allow` is a
 * bitmap of uint32 words: row i is allowed iff bit (i & 31) of word (i >> 5) is set -- numpy's
 * packbits(bitorder="little") read as little-endian words.  It is read in its first ceil(size / 32)
 * words only, bits at and past `size` in the last word are ignored, it needs 4-byte alignment, one
 * bitmap serves all queries of the call, and NULL means live rows only.  The host form takes a host
 * bitmap, the _device form a device bitmap on `device` (read on `stream`; it must stay valid and
 * unchanged until the search has run).  The filter is exact: the result is, bit for bit, the unfiltered
 * search of an index that holds only the allowed live rows, with its indices mapped back; a row that is
 * not allowed never enters a list (a NaN score does: it ranks below -inf).  Slots beyond
 * min(k, allowed live rows) hold (-1, -inf); an index whose rows are all removed or filtered out returns
 * only such slots and no error; size == 0 stays "Empty batch".  clipgpu_index_search[_device] are the
 * filtered forms with allow = NULL: they honour removals, and on an index without removed rows they
 * run the kernels they always ran.  The two bitmaps a search needs (live rows; live AND allow) are part
 * of the work area allocated at creation (capacity / 4 bytes together): a search still allocates nothing.
 *
 * Probabilities.  clipgpu_index_search_probs[_device] are the filtered forms with one more output, what
 * Clip::rank_images and Clip::classify return (src/clip.rs:92-170) for the k best rows: out_prob [nq][k].
 * Let A be the live rows that `allow` admits (NULL: every live row) and l_j the logit of row j as above.
 *   CLIPGPU_SIM_SOFTMAX: p_j = exp(l_j - M) / sum over i in A of exp(l_i - M), M = the largest l_i of A --
 *     the max-subtracted softmax over ALL rows of A, not over the k results, and over no other row: the
 *     result is that of an index holding only the rows of A.  The [nq][size] matrix still never exists:
 *     the kernels keep one running (max, sum) pair per query row beside the top-k selection.  In f32 with
 *     expf; the relative error of p_j and of the sum against exact arithmetic on the same logits is bounded
 *     in DESIGN.md (embedding index, probabilities): below 2^-12 up to |l - M| <= 200 and a million rows.
 *     out_norm (NULL = not wanted) receives (M, S) per query, S = sum exp(l_i - M) >= 1, so that the
 *     probability of ANY row is exp(l - M) / S (and a sharded gallery can combine its parts).
 *   CLIPGPU_SIM_SIGMOID: p_j = 1 / (1 + expf(-l_j)), bit-identical to clipgpu_similarity(...,
 *     CLIPGPU_SIM_SIGMOID) at those entries; out_norm is left untouched.
 *   CLIPGPU_SIM_LOGITS or an unknown activation: CLIPGPU_ERR_INVALID, before any device call.
 * out_idx and out_score are exactly those of clipgpu_index_search_filtered, in the same order; the empty
 * slots beyond min(k, |A|) hold probability 0 (with A empty: every slot, out_norm = (-inf, 0), no error).
 * A NaN or +inf logit in A makes every softmax probability of that query NaN, as the reference's
 * exp(x - max) does; -inf logits add nothing (all of A at -inf: NaN, as there).  Mutex, event ordering,
 * chunking, host staging and "the _device form does not synchronise" are those of the other searches;
 * the pairs (at most 512 KiB) and the staged outputs are part of the work area allocated at creation.
 *
 * Range search and duplicate pairs.  clipgpu_index_range_search[_device] return EVERY live allowed row whose
 * score against a query is >= threshold (an f32 comparison of the score above, bit-identical to the search's
 * and to clipgpu_similarity's logits; a NaN score never passes, not even at threshold = -inf), for callers
 * who know a score and not a k.  `allow` / `d_allow` as in the filtered search.
 *   _device form: records (query index, gallery row, score) go to d_out_query / d_out_row / d_out_score
 *     (device arrays of `capacity` entries each, 12 bytes per record together) in NO particular order, and
 *     *d_out_total (device, 8-byte aligned; zeroed by the call on `stream`) counts every hit, past the
 *     capacity too.  Once `stream` has run, min(total, capacity) records are valid; if total <= capacity they
 *     are the complete set.  No record is ever written at or past `capacity`.  Ordered after the handle's last
 *     operation; does not synchronise.
 *   host form: CSR.  out_lims [nq + 1]; query q's results are out_idx / out_score [out_lims[q], out_lims[q+1])
 *     in the search's order (descending score, equal scores by ascending row); out_idx and out_score have
 *     max_results entries.  *out_total is written whenever the device work ran.  total > max_results is
 *     CLIPGPU_ERR_INVALID with a message that names both numbers; the output arrays are then unspecified and
 *     the caller retries with max_results >= *out_total.  The records pass through a device buffer of
 *     max_results * 12 bytes that the handle allocates at the first such call, grows when a later call asks
 *     for more and keeps until it is destroyed (a failed allocation is CLIPGPU_ERR_DEVICE and leaves the
 *     index usable), and through twice those bytes of host memory for the sort.
 *   clipgpu_index_self_join: the gallery against itself, every pair i < j of live allowed rows with
 *     score(i, j) >= threshold, sorted by (i, j) ascending, out_i / out_j / out_score [max_pairs]; overflow,
 *     *out_total and the record buffer as in the host form above.  Rows i are read as stored (a 16-bit
 *     gallery: widened, exactly), so (i, j) carries exactly clipgpu_similarity(rows, rows)[i][j] of the
 *     stored rows -- the product chain does not care which side is which, the score is symmetric bit for bit.
 *     With logit_scale 1 and logit_bias 0 on L2-normalised rows the threshold is a cosine.
 * Limits, refused with CLIPGPU_ERR_INVALID before any device call: a NULL handle or output, nq <= 0 or an
 * empty index ("Empty batch"), nq > 2^31 - 1 (a record holds an int32 query index), a NaN threshold, and
 * capacity / max_results / max_pairs outside 1 .. 2^28 (2^28 records are 3 GiB of device memory and, for
 * the host forms, twice that in host memory while they sort).
 *
 * Assignment and k-means.  clipgpu_index_assign[_device] give, for every slot j < size, the nearest of C
 * centroids (f32 [C][E] whatever the gallery's type; the _device form wants them 16-byte aligned):
 *   label[j] = the centroid a clipgpu_index_search with k = 1 of an index holding the C centroids returns for
 *     the query g_j (row j as stored): the highest score, equal scores to the lower centroid index, a NaN
 *     below -inf; score[j] = fmaf(dot(c_label, g_j), logit_scale, logit_bias) with the bits of
 *     clipgpu_similarity(centroids, rows, logits)[label][j] (the score is symmetric bit for bit);
 *   a row that is dead or not allowed (`allow` / `d_allow` as in the filtered search) gets (-1, -inf), the
 *     search's empty entry.  Nothing at or past `size` is written.
 *   _device form: d_label int32 [size], d_score f32 [size]; ordered after the handle's last operation, does
 *     not synchronise.  Host form: out_label int64 [size], out_score f32 [size]; the centroids, labels and
 *     scores pass through buffers the handle allocates at the first such call, grows on demand and keeps
 *     until it is destroyed (a failed allocation is CLIPGPU_ERR_DEVICE and leaves the index usable).
 *   One launch covers the gallery: a block owns 64 rows and walks all centroids, so there is no span cut,
 *     no row chunk and no merge, and clipgpu_test_topk_span_cols / clipgpu_test_topk_route change nothing.
 * clipgpu_index_kmeans runs spherical Lloyd iterations over the live allowed rows, from the C centroids in
 * `centroids` (host, in: the start, out: the result), with logit_scale 1 and logit_bias 0 (cosines on unit
 * rows).  With n = the live allowed rows:
 *   for t = 1, 2, ...: labels_t = assign(centroids_{t-1}); moved_t = the live allowed rows whose label differs
 *     from labels_{t-1} (moved_1 = n); moved_t == 0: stop, iters = t, the centroids untouched; else
 *     centroids_t = update(labels_t); t == max_iter: stop, iters = max_iter, after one more assign -- the
 *     labels and scores returned are ALWAYS exactly assign(the centroids returned).
 *   out_moved[t - 1] = moved_t, entries past iters are -1; out_count[c] = the rows whose returned label is c.
 *   update, in integers, so that it does not depend on the order rows are met in (a repeated run, a permuted
 *     gallery and another grid give the same bits; a converged result is an exact fixed point):
 *       m = the largest |x| over the live allowed rows as stored; e = frexp(m)'s exponent (0 if m == 0);
 *       b = the bit length of n; s = 62 - e - b, so that |sum| < 2^62 always;
 *       S[c][i] = sum over label_j == c of llrint(ldexp((double)g_j[i], s)), int64, round to nearest even;
 *       with v_i = (double)S[c][i] and n2 = sum_i v_i * v_i in f64 (i ascending, multiply and add rounded
 *       separately): if n2 > 0, centroid[c][i] = (float)(v_i / sqrt(n2)), correctly rounded divide and root.
 *     A cluster with no member, or whose members sum to zero, keeps its previous centroid bit for bit (its
 *     count says which): re-seeding is the caller's business.
 *   A non-finite element in a live allowed row is CLIPGPU_ERR_INVALID, the message names the first such row.
 *   The call holds the handle's mutex throughout and synchronises once per iteration (it reads moved_t).
 *   Buffers as the host assign's, plus the sums (C * E * 8 bytes).
 * clipgpu_index_get_rows_at copies the rows at ids[0 .. n) (host; dead rows and repeats allowed; the range
 * rules of clipgpu_index_set_rows) as stored, widened to f32, in the order of ids, to out_rows [n][E] (host):
 * what a caller seeds k-means with.
 * Refused with CLIPGPU_ERR_INVALID before any device call: a NULL handle, input or output; C outside
 * 1 .. 65536; max_iter < 1; an empty index ("Empty batch").
 *
 * Inverted lists and the probed search (IVF).  clipgpu_index_partition fixes, at the moment it is called,
 *   label[j] = the label clipgpu_index_assign(centroids, 1.0, 0.0, NULL) returns for row j, for every live row
 *     j < size (exactly one label >= 0 each; a row with NaN scores still has a largest key), and
 *   list c   = the live rows with label c, ids ascending; a row dead at that moment is in no list.
 * centroids: host f32 [C][E], copied into the handle; 1 <= C <= 65536; out_counts (NULL = not wanted) receives
 * the C list lengths.  The lists are a pure function of the labels (a stable counting sort on the device: the
 * same bits on every run).  The call synchronises.  clipgpu_index_partition_lists returns C, 0 if there is no
 * partition, -1 if it is stale; clipgpu_index_get_lists copies the CSR to the host: out_offsets int64 [C + 1],
 * out_ids int64 [out_offsets[C]] (the caller sizes it with size, or from the counts); clipgpu_index_drop_partition
 * forgets the partition.
 *   clipgpu_index_search_probed[_device] return, for each query q, bit for bit what
 * clipgpu_index_search_filtered(q, k, logit_scale, logit_bias, allow = A_q) returns, where A_q is the set of
 * rows that are live now, allowed by `allow` (as in the filtered search) and whose label is in P_q, and P_q is
 * the index set a clipgpu_index_search with k = min(nprobe, C), scale 1, bias 0 of an F32 index holding the C
 * centroids returns for q (the largest keys; equal scores to the lower centroid).  The result carries the
 * original row ids and the scores' own bits, (-1, -inf) past min(k, |A_q|), and equal scores come out by
 * ascending row id whatever list or position the rows sit in.  It is approximate only in which rows it looks at.
 * 1 <= nprobe <= CLIPGPU_TOPK_MAX; nprobe >= C is the filtered search, exactly.  out_probes / d_probes (NULL =
 * not wanted): int64 [nq][nprobe], P_q best first, -1 past min(nprobe, C).  A query reads its nprobe lists and
 * the C centroids instead of the gallery: per chunk of queries one coarse search of the handle's centroid copy,
 * one launch over (query, probed list, part of the list) and the search's merge, in the workspace allocated at
 * creation.  The _device form is ordered after the handle's last operation and does not synchronise.
 *   clipgpu_index_remove keeps the partition valid: the id stays in its list and is rejected by the live bit
 * at search time.  clipgpu_index_add, _add_device, _set_rows and _clear make it STALE: a probed search (and
 * clipgpu_index_get_lists) is then CLIPGPU_ERR_INVALID, before any device call, with a message that says
 * "stale"; with no partition at all the message says "no partition".  clipgpu_index_partition may be called
 * again at any time and replaces the old partition (an assignment plus the list build; there is no
 * incremental insertion).  The partition's buffers (ids and offsets, 4 bytes per row and list; the centroid
 * copy; 640 KiB for the coarse results) are allocated at the first partition, grown on demand and kept until
 * the handle is destroyed; the list build passes through the handle's scratch buffer (about 5 bytes per row).
 * Refused with CLIPGPU_ERR_INVALID before any device call: a NULL handle, input or output; C outside
 * 1 .. 65536; nq <= 0 or an empty index ("Empty batch"); k or nprobe outside 1 .. CLIPGPU_TOPK_MAX. */
typedef struct clipgpu_index clipgpu_index;
#define CLIPGPU_TOPK_MAX 128
enum clipgpu_index_dtype { CLIPGPU_INDEX_F32 = 0, CLIPGPU_INDEX_F16 = 1, CLIPGPU_INDEX_BF16 = 2 };
int clipgpu_index_create(int device, int64_t E, int64_t capacity, clipgpu_index** out);
int clipgpu_index_create_ex(int device, int64_t E, int64_t capacity, int dtype, clipgpu_index** out);
int clipgpu_index_dtype(const clipgpu_index* ix); /* the enum; -1 for NULL */
int clipgpu_index_get_rows(clipgpu_index* ix, int64_t first, int64_t n, float* out_rows); /* host [n][E] */
void clipgpu_index_destroy(clipgpu_index* ix);
int64_t clipgpu_index_size(const clipgpu_index* ix); /* rows added so far */
int clipgpu_index_clear(clipgpu_index* ix);          /* size 0; the capacity stays */
int clipgpu_index_add(clipgpu_index* ix, const float* rows, int64_t n); /* host rows [n][E] */
int clipgpu_index_add_device(clipgpu_index* ix, const float* d_rows, int64_t n, void* stream);
int clipgpu_index_search(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                         float logit_bias, int64_t* out_idx, float* out_score);
int clipgpu_index_search_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k, float logit_scale,
                                float logit_bias, int64_t* d_idx, float* d_score, void* stream);
int clipgpu_index_remove(clipgpu_index* ix, const int64_t* ids, int64_t n); /* host ids */
int64_t clipgpu_index_live(const clipgpu_index* ix);                         /* live rows, exactly */
int clipgpu_index_get_live(clipgpu_index* ix, int64_t first, int64_t n, uint8_t* out); /* host [n], 0 / 1 */
int clipgpu_index_set_rows(clipgpu_index* ix, const int64_t* ids, const float* rows, int64_t n); /* host */
int clipgpu_index_search_filtered(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                                  float logit_bias, const uint32_t* allow, int64_t* out_idx, float* out_score);
int clipgpu_index_search_filtered_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                         float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t* d_idx,
                                         float* d_score, void* stream);
int clipgpu_index_search_probs(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, float logit_scale,
                               float logit_bias, int activation, const uint32_t* allow, int64_t* out_idx,
                               float* out_score, float* out_prob, float* out_norm);
int clipgpu_index_search_probs_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                      float logit_scale, float logit_bias, int activation, const uint32_t* d_allow,
                                      int64_t* d_idx, float* d_score, float* d_prob, float* d_norm, void* stream);
int clipgpu_index_range_search_device(clipgpu_index* ix, const float* d_queries, int64_t nq, float threshold,
                                      float logit_scale, float logit_bias, const uint32_t* d_allow, int64_t capacity,
                                      int32_t* d_out_query, int32_t* d_out_row, float* d_out_score,
                                      uint64_t* d_out_total, void* stream);
int clipgpu_index_range_search(clipgpu_index* ix, const float* queries, int64_t nq, float threshold, float logit_scale,
                               float logit_bias, const uint32_t* allow, int64_t max_results, int64_t* out_lims,
                               int64_t* out_idx, float* out_score, int64_t* out_total);
int clipgpu_index_self_join(clipgpu_index* ix, float threshold, float logit_scale, float logit_bias,
                            const uint32_t* allow, int64_t max_pairs, int64_t* out_i, int64_t* out_j, float* out_score,
                            int64_t* out_total);
int clipgpu_index_get_rows_at(clipgpu_index* ix, const int64_t* ids, int64_t n, float* out_rows);
int clipgpu_index_assign_device(clipgpu_index* ix, const float* d_centroids, int64_t C, float logit_scale,
                                float logit_bias, const uint32_t* d_allow, int32_t* d_label, float* d_score,
                                void* stream);
int clipgpu_index_assign(clipgpu_index* ix, const float* centroids, int64_t C, float logit_scale, float logit_bias,
                         const uint32_t* allow, int64_t* out_label, float* out_score);
int clipgpu_index_kmeans(clipgpu_index* ix, int64_t C, float* centroids, int64_t max_iter, const uint32_t* allow,
                         int64_t* out_label, float* out_score, int64_t* out_count, int64_t* out_moved,
                         int64_t* out_iters);
int clipgpu_index_partition(clipgpu_index* ix, const float* centroids, int64_t C, int64_t* out_counts);
int64_t clipgpu_index_partition_lists(const clipgpu_index* ix); /* C; 0 = no partition; -1 = stale */
int clipgpu_index_get_lists(clipgpu_index* ix, int64_t* out_offsets, int64_t* out_ids);
int clipgpu_index_drop_partition(clipgpu_index* ix);
int clipgpu_index_search_probed(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, int64_t nprobe,
                                float logit_scale, float logit_bias, const uint32_t* allow, int64_t* out_idx,
                                float* out_score, int64_t* out_probes);
int clipgpu_index_search_probed_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                       int64_t nprobe, float logit_scale, float logit_bias, const uint32_t* d_allow,
                                       int64_t* d_idx, float* d_score, int64_t* d_probes, void* stream);

/* ---- int8 codes and the coded search: a coarse scan of a compressed copy, then an exact re-rank ----------
 * clipgpu_index_enable_codes allocates, beside the gallery, int8 codes [capacity][Ep] (Ep = E rounded up to 64,
 * the bytes past E zero) and one f32 scale per row -- capacity * (Ep + 4) bytes, a quarter of an f32 gallery --
 * and codes rows [0, size).  From then on add, add_device and set_rows code the rows they write (same stream,
 * after the gallery write); clear keeps the codes enabled; remove needs nothing.  Enabling twice is a no-op;
 * drop_codes frees them.  E > 1024 is refused.  The code of a row x, as stored and widened to f32 (a 16-bit
 * index codes its rounded rows), every step one f32 operation:
 *   m = max |x_i|;  if m is not finite (an inf or a NaN anywhere in the row), m == 0 or 127 / m is not finite:
 *   every code 0 and scale 0;  else inv = 127 / m, code_i = clamp(rint(x_i * inv), -127, 127) with rint to
 *   nearest even, scale = m / 127 (both divisions correctly rounded).
 * get_codes copies rows [first, first + n) out: out_codes int8 [n][E], out_scales f32 [n].
 *
 * clipgpu_index_search_coded: the queries are coded by the same rule; for query q and live allowed row j
 *   coarse[q][j] = (float)(sum_i cq_i * cg_i) * scale[j]     (an exact int32 sum, one f32 multiply),
 * negated when logit_scale < 0 (0 counts as positive).  The candidates of q are the `refine` rows with the
 * largest (coarse, then lower row) in the search's order; the result is, bit for bit -- ids, order, score bits,
 * (-1, -inf) padding -- what clipgpu_index_search_filtered returns with allow = those candidates: approximate
 * only in which rows reach the exact re-rank.  If at most `refine` rows are live and allowed it is the plain
 * search.  1 <= k <= refine <= CLIPGPU_TOPK_MAX.  out_cand (int64 [nq][refine], -1 padded) and out_coarse (f32
 * [nq][refine], -inf padded) receive the candidates and their coarse scores, best first, or are NULL.
 * Refused before any device call: a NULL argument, an empty batch, k or refine out of range, an index without
 * codes.  The device form never synchronises and is ordered like clipgpu_index_search_probed_device. */
int clipgpu_index_enable_codes(clipgpu_index* ix);
int clipgpu_index_has_codes(const clipgpu_index* ix);
int clipgpu_index_drop_codes(clipgpu_index* ix);
int clipgpu_index_get_codes(clipgpu_index* ix, int64_t first, int64_t n, int8_t* out_codes, float* out_scales);
int clipgpu_index_search_coded(clipgpu_index* ix, const float* queries, int64_t nq, int64_t k, int64_t refine,
                               float logit_scale, float logit_bias, const uint32_t* allow, int64_t* out_idx,
                               float* out_score, int64_t* out_cand, float* out_coarse);
int clipgpu_index_search_coded_device(clipgpu_index* ix, const float* d_queries, int64_t nq, int64_t k,
                                      int64_t refine, float logit_scale, float logit_bias, const uint32_t* d_allow,
                                      int64_t* d_idx, float* d_score, int64_t* d_cand, float* d_coarse, void* stream);

/* ---- data-parallel sharding + the RCCL all-gather (north_star: "batches shard
 * data-parallel across the 8 GPUs of one node with an RCCL all-gather over xGMI only for the final
 * embedding matrix").  The reference has no multi-device path: embed_images / embed_texts
 * (src/vision.rs:100-117, src/text.rs:148-169) keep their signatures; these entry points are
 * what a multi-GPU caller of them binds.
 * Communicator: a handle created over n > 1 DISTINCT devices owns one (ncclCommInitAll, rank i =
 * device_ids[i]), created on its first gathered call (or at creation with
 * clipgpu_options.communicator = 1), so creation and the host-buffer entry points never depend
 * on RCCL; a one-device handle in a one-process-per-GPU deployment joins one with
 * clipgpu_comm_init_rank (rank 0 calls clipgpu_comm_unique_id and sends the 128 bytes to every
 * rank out of band; every rank then calls init_rank, collectively).  clipgpu_comm_info gives
 * (nranks, first rank of this handle); nranks 0 = no communicator.
 * Gathered forward: rows[nranks] = every rank's block size (identical on every rank); per LOCAL
 * device i (rank = first rank + i): d_in[i] = that rank's block on device i (f32 NCHW normalised
 * pixels / i64 ids [rows][T]), d_out[i] = [sum rows][E] f32 on device i, streams[i] (a NULL entry, or
 * a NULL array: device i's legacy default stream, as for the single-device *_device entry points).
 * Each rank embeds its block into its slot, then one collective
 * (in-place ncclAllGather for equal blocks; one ncclBroadcast per block otherwise) leaves the
 * whole matrix in rank order on every device.  Stream-ordered; collective over all ranks. */
int clipgpu_comm_unique_id(uint8_t* id /* [128] */);
int clipgpu_comm_init_rank(clipgpu_engine* e, const uint8_t* id /* [128] */, int nranks, int rank);
int clipgpu_comm_info(const clipgpu_engine* e, int* nranks, int* rank0);
int clipgpu_embed_pixels_gather_device(clipgpu_engine* e, const float* const* d_nchw, const int64_t* rows,
                                       float* const* d_out, void* const* streams);
int clipgpu_embed_tokens_gather_device(clipgpu_engine* e, const int64_t* const* d_ids, const int64_t* rows,
                                       float* const* d_out, void* const* streams);

/* ---- Clip facade scores on the host, the reference's f32 arithmetic bit for bit -----------
 * src/clip.rs:79-185 as the crate computes it (ndarray 0.17 without BLAS, Cargo.toml:14):
 * out[i] = unrolled_dot(embs[i], query).mul_add(logit_scale, logit_bias) -- ndarray's
 * eight-accumulator numeric_util::unrolled_dot, one fused multiply-add -- then
 *   CLIPGPU_SIM_SOFTMAX: max (f32::max fold) -> exp(x - max) -> sequential f32 sum -> x / sum
 *     over the n scores (classify :92-132 with embs = label embeddings, query = the image;
 *     rank_images :134-170 with embs = image embeddings, query = the text);
 *   CLIPGPU_SIM_SIGMOID: 1 / (1 + exp(-l)) (:181-185);  CLIPGPU_SIM_LOGITS: the logits (compare,
 *     :79-90, n = 1).
 * embs [n][E], query [E], out [n] f32; no GPU involved.  n == 0 -> "Empty batch". */
int clipgpu_facade_scores(const float* embs, int64_t n, const float* query, int64_t E, float logit_scale,
                          float logit_bias, int activation, float* out);

/* ---- live kernel timing -------------------------------------------------------------------
 * Records HIP events around every launch whose category bit is set in `mask` (on the launch
 * stream), for the device-resident entry points.  Categories: 0 patch_embed, 1 stem_ln, 2 qkv,
 * 3 attention, 4 out_proj, 5 layernorm, 6 c_fc, 7 c_proj, 8 head, 9 last_layer (the pruned
 * last layer's gather, out_proj, ln_2, c_fc and c_proj at M = batch).  enable() resets totals;
 * read() waits for the recorded events and returns the summed ms and launch count.  While a
 * mask is set, a batch's concurrent sub-batch lanes run one after another on the launch
 * stream (same launches, no overlap), so each event pair times one kernel alone -- unless the
 * mask also has CLIPGPU_PROFILE_CONCURRENT: then the lanes stay concurrent (no graph replay) and
 * each GEMM's event pair times its launch beside the other lane's kernels, as in the timed step. */
#define CLIPGPU_PROFILE_CONCURRENT 0x80000000u
int clipgpu_profile_enable(clipgpu_engine* e, unsigned mask);
int clipgpu_profile_read(clipgpu_engine* e, int category, double* total_ms, int64_t* launches);
const char* clipgpu_profile_category_name(int category);

/* ---- test hooks --------------------------------------------------------------------------
 * The seeded weight generator shared with the oracle (bit-exact). */
int clipgpu_synth_tensor(uint64_t seed, const char* name, double std, double offset, float* out, int64_t n);

#ifdef __cplusplus
}
#endif

#endif /* CLIPGPU_H */
