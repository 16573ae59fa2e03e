/*
 * include/fleet_codec.h -- C-ABI of the MI355X-native FLeet gradient codec and
 * server-side aggregation path (libfleetcodec.so).
 *
 * This is the drop-in boundary under the reference's JNI layer. Every entry
 * point below replaces a native function of the reference's server backend
 * (libnative.so built from Server/src/main/c++/cppNN_backend.cpp), or the
 * call sequence CppNNUpdater.update drives through them, and produces the
 * same bytes. The JNI shim (fleet_amd/csrc/jni_shim.cpp, libfleet_native.so)
 * re-exports the reference's Java_* symbols on top of this ABI; see
 * INTEGRATION.md for the Java-side binding.
 *
 * Conventions
 *   - Plain pointers and sizes; no torch/HIP types. `stream` arguments are a
 *     hipStream_t passed as void* (NULL = the null/default stream). Host-buffer
 *     entry points run on the context's own stream and return synchronously.
 *   - "Base64" buffers are the reference's wire format: Base64 (RFC 4648
 *     alphabet; '-' and '_' accepted as 62/63 on input, from_base64 at Base64.cpp:20-27) of
 *     little-endian int32 decimal fixed-point codes (Base64::float2int,
 *     Base64.cpp:48-78). Host buffers are NOT NUL-terminated.
 *   - Every function returns FLEET_OK (0) or a negative FLEET_ERR_* code;
 *     fleet_last_error() gives a message. The reference has no error
 *     reporting (malformed input is UB there); here it is rejected.
 *   - Thread safety: a context serialises its own calls with an internal
 *     mutex (the reference serialises all updater natives under
 *     `synchronized(acc)`, CppNNUpdater.java:259,333). Use one context per
 *     thread/GPU for concurrency.
 *   - Input contract: Base64 text produced by Base64::encode -- length a
 *     multiple of 4, '=' only as trailing padding. Anything else returns
 *     FLEET_ERR_BASE64 (the reference would silently drop bytes).
 */
#ifndef FLEET_CODEC_H
#define FLEET_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLEET_OK 0
#define FLEET_ERR_ARG (-1)      /* bad argument / size mismatch */
#define FLEET_ERR_BASE64 (-2)   /* text outside the Base64::encode output contract */
#define FLEET_ERR_LAYOUT (-3)   /* gradient layout header inconsistent (network.h:1038-1056) */
#define FLEET_ERR_HIP (-4)      /* HIP runtime failure (or no GPU) */
#define FLEET_ERR_NOMEM (-5)
#define FLEET_ERR_CAPACITY (-6) /* output buffer too small; *out_len holds the size needed */

#define FLEET_MAX_HEADERS 4096

typedef struct fleet_ctx fleet_ctx;

/* Library / context ------------------------------------------------------ */
const char* fleet_version(void);
int fleet_create(int device, fleet_ctx** out);
void fleet_destroy(fleet_ctx* ctx);
const char* fleet_last_error(const fleet_ctx* ctx);
int fleet_sync(fleet_ctx* ctx, void* stream);
/* the HIP device the context was created on (-1 for NULL) */
int fleet_ctx_device(const fleet_ctx* ctx);

/* Base64 length of n int32/fp32 values: 4*ceil(4n/3) (Base64.cpp:129-136). */
size_t fleet_b64_len(size_t n_values);
/* Number of int32 values carried by a Base64::encode output of length len. */
size_t fleet_b64_count(size_t len);

/* Gradient layout (network.h:1038-1056): [nW,(size_i,dW_i..)*,nB,(size_j,db_j..)*].
 * Writes the sorted header slot positions; returns FLEET_OK and *n_headers,
 * *n_up (total floats). */
int fleet_layout_from_sizes(const int32_t* w_sizes, int n_w, const int32_t* b_sizes, int n_b,
                            int32_t* header_pos, int cap, int* n_headers, size_t* n_up);
/* Same, parsed from an upload (Base64 host buffer) by decoding its header
 * slots on the device, exactly as network::flatGrad walks them (:1206-1223).
 * *n_up = the floats the walk covers (= the upload's count for gradients()
 * output); slots past it are carried from the last upload, like headers. */
int fleet_layout_parse(fleet_ctx* ctx, const char* upload, size_t len, int32_t* header_pos, int cap,
                       int* n_headers, size_t* n_up);

/* Codec (Base64.cpp) -- host buffers ------------------------------------- */
/* Base64::encode(std::vector<float>) (:140-142) */
int fleet_encode_f32(fleet_ctx* ctx, const float* values, size_t n, char* out, size_t cap, size_t* out_len);
/* Base64::encode(std::vector<int>) (:145-151) */
int fleet_encode_i32(fleet_ctx* ctx, const int32_t* codes, size_t n, char* out, size_t cap, size_t* out_len);
/* Base64::decodeFloat (:207-209) */
int fleet_decode_f32(fleet_ctx* ctx, const char* text, size_t len, float* out, size_t cap, size_t* n_out);
/* Base64::decodeInt (:211-219) */
int fleet_decode_i32(fleet_ctx* ctx, const char* text, size_t len, int32_t* out, size_t cap, size_t* n_out);

/* Per-op JNI replacements (cppNN_backend.cpp) -- host Base64 buffers ------ */
/* Java_apps_cppNN_CppNNUpdater_getFlatGradient (:701-720) */
int fleet_flat_gradient(fleet_ctx* ctx, const char* g, size_t len, char* out, size_t cap, size_t* out_len);
/* Java_apps_cppNN_CppNNUpdater_mergeFlatGradient (:722-750) */
int fleet_merge_flat_gradient(fleet_ctx* ctx, const char* g, size_t glen, const char* flat, size_t flen,
                              char* out, size_t cap, size_t* out_len);
/* Java_utils_ByteVec_scalarMulNative (:753-777) */
int fleet_scalar_mul(fleet_ctx* ctx, const char* v, size_t len, double a, char* out, size_t cap,
                     size_t* out_len);
/* Java_utils_ByteVec_addNative (:797-846) */
int fleet_add(fleet_ctx* ctx, const char* a, size_t alen, const char* b, size_t blen, char* out, size_t cap,
              size_t* out_len);
/* Java_utils_ByteVec_subtractNative (:848-892) */
int fleet_subtract(fleet_ctx* ctx, const char* a, size_t alen, const char* b, size_t blen, char* out,
                   size_t cap, size_t* out_len);
/* Java_utils_ByteVec_getNorm (:779-795): sqrt(sum_i (double)(x_i*x_i)) in index order */
int fleet_norm(fleet_ctx* ctx, const char* v, size_t len, double* out);

/* The fused update -- host buffers ---------------------------------------
 * One call = the aggregation part of CppNNUpdater.update (CppNNUpdater.java:
 * 420-509): for the M picked uploads in order,
 *   pickedGrad = getFlatGradient(g_i).scalarMultiply(dampen[i]); avg += pickedGrad
 *   merged = mergeFlatGradient(g_{M-1}, avg.scalarMultiply(1.0/M))
 * with every intermediate re-quantised exactly as the per-op JNI chain does.
 * All uploads must share one layout and length. `merged` receives the
 * Base64 the reference returns; `merged_f32` (nullable, n_up floats) receives
 * Base64::decodeFloat(merged), i.e. what descentNative decodes (:336). */
int fleet_update(fleet_ctx* ctx, const char* const* uploads, const size_t* lens, int M, const double* dampen,
                 char* merged, size_t cap, size_t* out_len, float* merged_f32);
/* The same update spread over the GPUs of a node from ONE host process
 * (SURVEY.md §8e element sharding; the reference server is one JVM calling
 * its natives under synchronized(acc), CppNNUpdater.java:333,420-509).
 * ctxs = n_ctx distinct contexts, one per device. Context k takes a
 * contiguous, balanced range of the 16-char / 3-value groups: on its own
 * thread it copies that column window of every upload into its pinned
 * staging, H2Ds it over its own PCIe link, runs the exact chain there and
 * D2Hs its merged slice straight into `merged` / `merged_f32` (disjoint byte
 * ranges). No collective and no reduction crosses devices, so the output is
 * byte-identical to fleet_update's. Errors are reported on ctxs[0]
 * (fleet_last_error), Base64 errors first. */
int fleet_update_multi(fleet_ctx* const* ctxs, int n_ctx, const char* const* uploads, const size_t* lens, int M,
                       const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32);
/* fleet_update / fleet_update_multi over uploads stored as M rows `row_pitch`
 * bytes apart (row i = upload i, `len` Base64 chars): the ingress of a caller
 * that deserialises the uploads into one buffer (a Java direct ByteBuffer,
 * INTEGRATION.md). When the whole row range lies inside ONE live
 * fleet_host_register registration every context DMAs its column window
 * straight from it -- no host copy at all; otherwise the rows are staged as
 * in fleet_update. */
int fleet_update_rows(fleet_ctx* ctx, const char* rows, size_t row_pitch, size_t len, int M, const double* dampen,
                      char* merged, size_t cap, size_t* out_len, float* merged_f32);
int fleet_update_rows_multi(fleet_ctx* const* ctxs, int n_ctx, const char* rows, size_t row_pitch, size_t len, int M,
                            const double* dampen, char* merged, size_t cap, size_t* out_len, float* merged_f32);
/* Page-lock (hipHostRegister, portable to every device) / release a long-lived
 * host buffer, e.g. the upload rows of fleet_update_rows. The registrations
 * are tracked process-wide: registering a range that overlaps a recorded
 * registration releases the old one first. Contract: unregister BEFORE the
 * memory is freed. The library cannot tell a registration whose memory was
 * freed and reused (a collected Java direct buffer, a new allocation at the
 * same addresses) from a live one: rows inside it would be DMA'd from the
 * stale pinned pages. */
int fleet_host_register(fleet_ctx* ctx, void* ptr, size_t bytes);
int fleet_host_unregister(fleet_ctx* ctx, void* ptr);
/* How the last host-buffer update on ctx (fleet_update*, its window on this context)
 * reached HBM: FLEET_INGRESS_STAGED (copied into the context's pinned staging),
 * FLEET_INGRESS_PINNED (one DMA straight from registered rows), or
 * FLEET_INGRESS_NONE before any. ctx NULL: the process's most recent such update
 * on any context (e.g. those of the JNI shim). Diagnostics and tests. */
#define FLEET_INGRESS_NONE 0
#define FLEET_INGRESS_STAGED 1
#define FLEET_INGRESS_PINNED 2
int fleet_last_ingress(fleet_ctx* ctx);

/* Device-resident entry points (all buffers are device pointers) ----------
 * Uploads are stored as M rows of `pitch` bytes (pitch >= 16*ceil(len/16),
 * multiple of 16); each row holds `len` Base64 chars. group_begin/group_end
 * select the 16-char / 3-value groups this call processes (element-range
 * sharding; [0, ceil(len/16)) = everything). `dampen` is a host array of M
 * doubles. Outputs are written for the selected groups only: merged Base64
 * at byte 16*g, merged_f32 (nullable) at value 3*g.
 * Only bytes [16*group_begin, 16*group_end) of each row (and of d_merged,
 * values [3*group_begin, 3*group_end) of d_merged_f32) are dereferenced, so a
 * rank holding just its window of every upload passes the window's address
 * minus 16*group_begin (3*group_begin floats for merged_f32) and pitch >=
 * 16*(group_end - group_begin): fleet_amd/shard.py does exactly that.
 * header_pos (a host array, whole-upload coordinates, at most FLEET_MAX_HEADERS
 * entries; fleet_layout_from_sizes / fleet_layout_parse produce it) holds
 * strictly ascending positions inside [0, fleet_b64_count(len)): the kernels
 * search the list. fleet_update_device, fleet_update_encode_device,
 * fleet_update_kardam_device, fleet_acc_create and fleet_pool_create return FLEET_ERR_ARG for any
 * other list (unsorted, duplicate, negative, past the upload) and launch
 * nothing; the context's resident parameters stay those of the last accepted
 * call. The list is checked when it differs from the resident one, so a
 * steady-state call makes no extra pass over it. fleet_synth(_window)_device's
 * header_pos are store targets in the tensor's own columns: each inside
 * [0, n_up), any order, header_pos and header_val non-NULL when n_headers > 0,
 * else FLEET_ERR_ARG before anything is allocated or launched.
 * Graph capture: the dampen and header words live in ONE device buffer per
 * context, re-uploaded (synchronously) whenever a call passes different ones.
 * Every graph captured on the context therefore replays with the parameters of
 * the context's latest call, and a capture cannot introduce new parameters
 * (FLEET_ERR_ARG): make one eager call with them first, and do not change them
 * while captured graphs that must keep the old ones are still replayed. */
int fleet_update_device(fleet_ctx* ctx, const void* d_uploads, size_t pitch, size_t len, int M,
                        const double* dampen, const int32_t* header_pos, int n_headers, size_t group_begin,
                        size_t group_end, void* d_merged, void* d_merged_f32, void* stream);
/* A pipelined step of the device-resident path: fleet_update_device over the
 * whole uploads in d_uploads AND fleet_encode_device of the next batch's M rows
 * of fp32 (d_values, n values, vpitch floats per row) into d_next_uploads (same
 * pitch; must not overlap d_uploads), in ONE launch when the update runs on the
 * stream grid (the aggregation is VALU-bound, the client encode HBM-bound: they
 * share the CUs), else the two kernels back to back. Results equal the two
 * calls' results. Replaces nothing in the reference (its clients encode on
 * their own devices); the bench's steady-state step. */
int fleet_update_encode_device(fleet_ctx* ctx, const void* d_uploads, size_t pitch, size_t len, int M,
                               const double* dampen, const int32_t* header_pos, int n_headers, void* d_merged,
                               void* d_merged_f32, const void* d_values, size_t vpitch, void* d_next_uploads,
                               void* stream);
/* fleet_update_device plus Kardam's bookkeeping of the same picked uploads
 * (CppNNUpdater.java:463-481, Kardam.java:48-106) as side
 * outputs of the one pass over the uploads (no second read of them):
 *   G_c = decodeFloat(getFlatGradient(u_c).scalarMultiply(dampen[c]).scalarMultiply(lr))
 *   norm_g[c]    = G_c's getNorm
 *   norm_diff[c] = getNorm(g_c.subtract(prev_c)) when has_prev[c] (else NaN)
 * with prev_c = the worker's previous G (d_prev: M rows of vpitch floats in
 * upload coordinates, header slots ignored; NULL = none) and, when d_g_out is
 * given, this round's G written there in the same layout (the next round's
 * prev; d_g_out may be d_prev itself: G then replaces prev in place). Whole
 * uploads (all groups); synchronous (the norms are host outputs);
 * not for graph capture. Norms: fixed-order partial sums of the reference's
 * fp64 loop (1e-12 relative, like fleet_norm). */
int fleet_update_kardam_device(fleet_ctx* ctx, const void* d_uploads, size_t pitch, size_t len, int M,
                               const double* dampen, const int32_t* header_pos, int n_headers, double lr,
                               const void* d_prev, const uint8_t* has_prev, void* d_g_out, size_t vpitch,
                               void* d_merged, void* d_merged_f32, double* norm_g, double* norm_diff, void* stream);
/* Client-side encode of M fp32 buckets (rows of `n` floats, `vpitch` floats
 * apart) into Base64 rows of `pitch` bytes: Base64::encode(vector<float>) per row. */
int fleet_encode_device(fleet_ctx* ctx, const void* d_values, size_t n, size_t vpitch, int M, void* d_out,
                        size_t pitch, void* stream);
/* Base64 rows -> fp32 (decodeFloat) per row. */
int fleet_decode_device(fleet_ctx* ctx, const void* d_text, size_t len, size_t pitch, int M, void* d_values,
                        size_t vpitch, void* stream);
/* Deterministic synthetic gradient buckets on the device (SURVEY.md §8d value
 * mix; Philox4x32-10 keyed by seed, counter = (element, client)), with the
 * given layout's header values written in place. Rows of `vpitch` floats. */
int fleet_synth_device(fleet_ctx* ctx, uint64_t seed, int M, int client0, const int32_t* header_pos,
                       const float* header_val, int n_headers, size_t n_up, void* d_values, size_t vpitch,
                       void* stream);
/* The same for a column window of a larger synthetic problem: values n_up columns
 * from element elem0 (the counter is the global element index, so a rank's window
 * holds exactly the fixed problem's values there); header_pos in window coordinates,
 * each inside [0, n_up) (see the device-resident entry points above). */
int fleet_synth_window_device(fleet_ctx* ctx, uint64_t seed, int M, int client0, size_t elem0,
                              const int32_t* header_pos, const float* header_val, int n_headers, size_t n_up,
                              void* d_values, size_t vpitch, void* stream);
/* Returns FLEET_ERR_BASE64 / FLEET_ERR_LAYOUT if a device-resident call
 * (fleet_*_device) since the last check saw malformed text or a header that
 * differs from the last upload's (synchronises the stream), and clears the
 * flag. Device-resident calls keep their parameters and error flag in buffers
 * of their own, so host-buffer calls on the same context (its own stream) may
 * be issued while device-resident work is still in flight, and a grown
 * parameter buffer that a captured HIP graph may reference stays allocated
 * until fleet_destroy. */
int fleet_check(fleet_ctx* ctx, void* stream);

/* Streaming aggregation: each upload folded into a resident sum on arrival ----
 * CppNNUpdater.update is entered once per upload; it buffers the upload
 * (CppNNUpdater.java:383-391) and, once M have arrived, picks them in arrival
 * order (:420-421), dampens each (:463-464), sums, averages and merges them
 * (:490-508). The chain is serial over the picked uploads and independent per
 * element, so a fleet_acc runs one upload's step when that upload arrives and
 * keeps only the running sum: after the M-th arrival what is left is one
 * upload's copy, one step and the finish, and the device holds two fp32 states
 * and two upload rows instead of M rows. The bytes are fleet_update's. Valid
 * for the branch fleet_update covers (staleSize == 0: picking order = arrival
 * order; pruning thresholds 0), where getDampen's inputs (getCurrEpoch, the
 * global label vector) change only inside the M-th call (:502-504, descentNative),
 * so the factor known at arrival is the one the batch loop would compute. For
 * staleSize > 0 keep the uploads in a fleet_pool (below), which aggregates any
 * picked subset of them, with Kardam's side outputs from the pooled rows through a
 * fleet_kledger (further below); for pruning thresholds above 0 keep the batch entry
 * points.
 *
 * An accumulator belongs to its context (same mutex and device; destroy it
 * before fleet_destroy; errors through fleet_last_error(ctx)) and owns its memory
 * -- two state buffers, two device rows (the incoming and the last accepted
 * upload), two pinned host rows, its error word, the first upload's header
 * codes -- so fleet_update* calls on the same context are unaffected. `len`, the
 * header positions and the group window are fixed at creation; [0, ceil(len/16))
 * = everything. header_pos is, as for fleet_update_device, a layout that covers
 * the whole upload, and a window behaves exactly like fleet_update_device's: the
 * accumulator reads and writes only the window's bytes and values, so one rank
 * may hold one accumulator over its window. */
typedef struct fleet_acc fleet_acc;
int fleet_acc_create(fleet_ctx* ctx, size_t len, const int32_t* header_pos, int n_headers, size_t group_begin,
                     size_t group_end, fleet_acc** out);
void fleet_acc_destroy(fleet_acc* acc);
/* One arrival of CppNNUpdater.update (CppNNUpdater.java:383-391) with its pick's
 * step of the loop at :420-421, :463-464, :490-508 run at once; `upload` is the
 * whole upload (host buffer, `len` chars; another length is FLEET_ERR_ARG),
 * `dampen` its getDampen factor. Synchronous and transactional: the window's
 * bytes go through the spare pinned row to the spare device row, the step
 * writes the spare state, and only after the error word was read back clean do
 * the state and the "last upload" flip and the count grow. On FLEET_ERR_BASE64
 * or FLEET_ERR_LAYOUT (a header slot differs from the batch's first upload) the
 * accumulator is exactly as before the call. */
int fleet_acc_push(fleet_acc* acc, const char* upload, size_t len, double dampen);
/* The same step for an upload already in HBM (d_upload: the whole row, of which
 * only the window's bytes are read), on the caller's stream. Asynchronous, no
 * synchronisation: the window is copied device-to-device into the accumulator's
 * own spare row on that stream and folded, so the caller may reuse d_upload as
 * soon as the stream allows. Unlike fleet_acc_push it cannot wait to learn
 * whether the upload was sound, so it commits at once (state and last upload
 * flip, the count grows on return), and a bad upload leaves a STICKY error: once
 * it is known (fleet_acc_finish*, which read the error word, or a later push
 * that finds the word already written back) every further push and finish
 * returns that code until fleet_acc_reset. Not for graph capture. */
int fleet_acc_push_device(fleet_acc* acc, const void* d_upload, double dampen, void* stream);
/* Uploads folded since the last finish / reset (the reference's acc.size(),
 * CppNNUpdater.java:383-391); FLEET_ERR_ARG for NULL. */
int fleet_acc_count(const fleet_acc* acc);
/* The merged gradient of the uploads pushed since the last finish: the sum's
 * scalarMultiply(1.0 / count) merged into the last accepted upload (CppNNUpdater.java:
 * 490-508), fleet_update's `merged` (len chars; this accumulator's window of them)
 * and optionally decodeFloat(merged) in merged_f32. count == 0: FLEET_ERR_ARG.
 * On success the count returns to 0: the accumulator is ready for the next batch
 * (:420-421 leave `acc` empty). The host form is synchronous; the device form
 * writes Base64 at byte 16*g and fp32 at value 3*g of the caller's buffers
 * (fleet_update_device's addressing, d_merged >= 16*ceil(len/16) bytes) on
 * `stream` and synchronises it to read the error word. */
int fleet_acc_finish(fleet_acc* acc, char* merged, size_t cap, size_t* out_len, float* merged_f32);
int fleet_acc_finish_device(fleet_acc* acc, void* d_merged, void* d_merged_f32, void* stream);
/* Drops what was pushed (a half-filled batch, CppNNUpdater.java:383-391's `acc`
 * cleared) and clears a sticky error; waits for the accumulator's device work. */
int fleet_acc_reset(fleet_acc* acc);
/* Bursts: K >= 1 uploads that are at hand together (a server draining its request
 * queue, a device-side producer) folded in arrival order by one kernel per
 * fleet_acc_burst() uploads, the running value held in registers across the
 * clients, so the state is read and written once per launch instead of once per
 * upload. Each step is fleet_acc_push's, so the bytes are those of K single pushes;
 * dampen[k] is upload k's getDampen factor (the K factors travel in the kernel
 * arguments). FLEET_ERR_ARG, before anything is copied: K <= 0, a NULL array or entry,
 * lens[k] != len, and for the device forms with K > 1 a base or pitch that is not a
 * multiple of 16 or a pitch below 16*ceil(len/16) (rows 0..K-2 are read in place
 * with 16-byte loads; only row K-1's window is copied into the accumulator's spare
 * row, where the finish finds the last accepted upload).
 *
 * fleet_acc_push_many is synchronous and all-or-nothing: the windows go through
 * pinned staging to device staging (at most fleet_acc_burst() rows of the window's
 * 16*groups + 64 bytes each on both sides, grown on demand, kept until
 * fleet_acc_destroy; a burst longer than that is staged and launched in chunks), one
 * stream synchronisation reads the error word, and on FLEET_ERR_BASE64 or
 * FLEET_ERR_LAYOUT from any of the K uploads the state, the last row and the count
 * are exactly as before the call; on success the count grows by K. (DMA straight
 * from page-locked rows the caller registered is not offered.)
 * fleet_acc_push_many_device is asynchronous on the caller's stream and commits at
 * once, a bad upload leaving a sticky error, exactly like fleet_acc_push_device; the
 * caller may reuse d_uploads as soon as the stream allows. Not for graph capture.
 *
 * fleet_acc_push_finish* fold the burst and produce fleet_acc_finish's outputs in the
 * same launch: the last kernel applies the average and the merge to its registers and
 * stores no state (the arrival that completes a batch pays one launch, not two). Both
 * forms synchronise to read the error word, so both are transactional: on an error of
 * one of the K uploads nothing is committed, the count is unchanged and the outputs
 * are not meaningful; an error left by an earlier fleet_acc_push_device of the same
 * batch stays sticky and comes first. On success the count returns to 0. The device
 * form uses fleet_acc_finish_device's addressing.
 *
 * Resident bytes of an accumulator over G groups: two states (2 * 12 G), two device
 * rows and two pinned rows (4 * 16 G), and after a host burst of K uploads the staging,
 * min(K - 1, fleet_acc_burst()) rows of 16 G bytes in HBM and as many pinned. */
int fleet_acc_push_many(fleet_acc* acc, const char* const* uploads, const size_t* lens, int K, const double* dampen);
int fleet_acc_push_many_device(fleet_acc* acc, const void* d_uploads, size_t pitch, int K, const double* dampen,
                               void* stream);
int fleet_acc_push_finish(fleet_acc* acc, const char* const* uploads, const size_t* lens, int K, const double* dampen,
                          char* merged, size_t cap, size_t* out_len, float* merged_f32);
int fleet_acc_push_finish_device(fleet_acc* acc, const void* d_uploads, size_t pitch, int K, const double* dampen,
                                 void* d_merged, void* d_merged_f32, void* stream);
/* B: uploads folded per launch. */
int fleet_acc_burst(void);

/* Upload pool: arrivals kept in HBM, any picked subset aggregated ---------------
 * With staleSize > 0 the reference's `acc` persists across updates
 * (CppNNUpdater.java:383-411): at update time StalenessSimulator.stalenessSim
 * (StalenessSimulator.java:38-176) picks M of the buffered uploads in an order of
 * its own, leaves the rest buffered and discards those that are too old. A fold
 * cannot be undone, so a fleet_acc does not cover that branch, and the batch calls
 * pay the copy of all M picked rows after the last arrival. A fleet_pool is `acc`
 * itself kept in HBM: an upload goes into a slot when it arrives (fleet_pool_put*),
 * an update names any subset of occupied slots in any order with one getDampen
 * factor each (CppNNUpdater.java:420-421, 463-464) and produces fleet_update's
 * bytes for those uploads in that order (CppNNUpdater.java:490-508); after the last
 * arrival what is left is one row's copy and one fold over resident rows. An update
 * never frees a slot: the caller drops what it picked (fleet_pool_drop), unpicked
 * slots stay for later updates.
 *
 * A pool belongs to its context like an accumulator (same mutex and device; destroy
 * it before fleet_destroy; errors through fleet_last_error(ctx)). `len`, the header
 * positions, the group window and `slots` >= 1 are fixed at creation, with
 * fleet_acc_create's checks; a window behaves as the accumulator's: only the
 * window's bytes are stored, read and written. Resident bytes over G groups:
 * (slots + 1) rows of 16 G + 64 bytes (the extra row takes the host update's merged
 * bytes), one fp32 state of 12 G bytes (it carries the running value between the
 * launches of an update of more than fleet_acc_burst() picks; fewer picks move no
 * state), the header block, the first pick's header codes, one status word per slot
 * in HBM and pinned, and one pinned row. A failed allocation is FLEET_ERR_NOMEM and
 * leaves nothing behind. */
typedef struct fleet_pool fleet_pool;
int fleet_pool_create(fleet_ctx* ctx, size_t len, const int32_t* header_pos, int n_headers, size_t group_begin,
                      size_t group_end, int slots, fleet_pool** out);
void fleet_pool_destroy(fleet_pool* pool);
int fleet_pool_slots(const fleet_pool* pool);
/* 1 / 0; FLEET_ERR_ARG for NULL or a slot outside [0, slots). */
int fleet_pool_occupied(const fleet_pool* pool, int slot);
/* One arrival (CppNNUpdater.java:383-411: the upload joins `acc`): fleet_acc_push's
 * ingress without the fold. The window's bytes go through the pinned row to the
 * slot, in pieces whose copy to the device overlaps the next piece's host copy;
 * synchronous. A put into an occupied slot replaces the upload. FLEET_ERR_ARG: a NULL
 * argument, a slot outside [0, slots), a length other than `len`. The text is checked
 * when it is picked, not here (fleet_gate_put, below, checks it on arrival). */
int fleet_pool_put(fleet_pool* pool, int slot, const char* upload, size_t len);
/* The same for an upload already in HBM (d_upload: the whole row, of which only the
 * window's bytes are read): copied device-to-device on the caller's stream, no
 * synchronisation. Host forms issued later wait for device puts in flight. */
int fleet_pool_put_device(fleet_pool* pool, int slot, const void* d_upload, void* stream);
/* Frees a slot (a picked upload after its update, or one StalenessSimulator.java:38-176
 * discards as too old). */
int fleet_pool_drop(fleet_pool* pool, int slot);
/* Aggregates the uploads in slots picks[0..K) in that order with dampen[k]
 * (CppNNUpdater.java:420-421, 463-464, 490-508): fleet_update's `merged` for those
 * uploads in that order and optionally decodeFloat(merged) in merged_f32, header and
 * unwalked slots from the last pick. fleet_acc_burst() picks per launch, the slots and
 * factors in the kernel arguments. The host form writes this pool's window of `merged`
 * (len chars) and of merged_f32; the device form uses fleet_acc_finish_device's
 * addressing on `stream`. FLEET_ERR_ARG, before anything is launched and with the slot
 * status untouched: K <= 0, a NULL array, a pick outside [0, slots), a pick of an
 * unoccupied slot, a slot picked twice. A `cap` below len is FLEET_ERR_CAPACITY with
 * *out_len = len. Both forms clear the slot status, fold, and synchronise once to read
 * it. On FLEET_ERR_BASE64 (a picked upload is not Base64::encode output) or
 * FLEET_ERR_LAYOUT (a picked upload's header slots differ from the first pick's) the
 * outputs are not meaningful, the pool is exactly as before -- no slot changes, nothing
 * is dropped -- and fleet_pool_slot_status names the offending slots; BASE64 comes
 * before LAYOUT. An upload in an unpicked slot is not looked at. */
int fleet_pool_update(fleet_pool* pool, const int32_t* picks, int K, const double* dampen, char* merged, size_t cap,
                      size_t* out_len, float* merged_f32);
int fleet_pool_update_device(fleet_pool* pool, const int32_t* picks, int K, const double* dampen, void* d_merged,
                             void* d_merged_f32, void* stream);
/* The error bits the last update saw in the slot's upload: 1 = Base64, 2 = layout
 * header; 0 for a clean or unpicked slot. FLEET_ERR_ARG for NULL or a bad slot. */
int fleet_pool_slot_status(const fleet_pool* pool, int slot);

/* Arrival gate: an upload vetted when it arrives, beside an upload pool ----------
 * fleet_pool_put does not look at the text, so a malformed upload waits in its slot until
 * an update picks it, and that update pays its whole fold to fail. The reference does at
 * arrival what it can -- a gradient for the wrong model is dropped there
 * (CppNNUpdater.java:350-353) --, and fleet_acc_push checks an upload as it folds it. A
 * fleet_gate is that check for a pool: one device pass over one or more resident slots
 * (k_pool_vet) that folds nothing and says, per slot,
 *   status   FLEET_ERRBIT_BASE64 (1): the text is not Base64::encode output -- the verdict
 *            an update's fold would reach, character for character (a bad character in a
 *            position a ragged last group does not need passes, as there);
 *            FLEET_ERRBIT_LAYOUT (2): a header slot's code differs from the code this
 *            model's gradients carry there (below); 0: the upload is good;
 *   sumsq    sum (double)(y * y) over the flat gradient, y = Q(dec(code)): the square of
 *            new ByteVec(getFlatGradient(g)).getNorm() (cppNN_backend.cpp:701-720, 779-795;
 *            getNorm's fp32 products summed in double, per wave and then the waves in a
 *            fixed order: no floating-point atomics, the same bits for the same upload
 *            whatever else is vetted beside it);
 *   max_abs  max |y| over the flat gradient.
 * With a windowed pool the results cover the window's slots alone, which is why the sum of
 * squares is returned and not its root: the windows of an upload add (and max_abs is the
 * largest of theirs).
 *
 * A gate belongs to one pool (same context, mutex and device; destroy it before
 * fleet_pool_destroy; errors through fleet_last_error(ctx)). It owns the expected header
 * codes, one launch's status words (fleet_acc_burst()) and per-wave partials (grid x 4 waves
 * x fleet_acc_burst() slots x 2 doubles), and status, sumsq and max_abs of max(slots,
 * fleet_acc_burst()) slots in HBM and pinned: nothing is allocated after create. A failed
 * allocation is FLEET_ERR_NOMEM and leaves nothing behind. The gate reads the pool's rows
 * and writes none of the pool's rows, state, first-pick header codes or slot status:
 * fleet_pool_slot_status keeps meaning "what the last update saw".
 *
 * Not built: JNI natives (the shim has no pool), a multi-GPU form, any change to
 * fleet_pool_put itself, and overlapping the vet with the put's copy pieces. */
typedef struct fleet_gate fleet_gate;
/* float2int of each value (Base64.cpp:60-73), on the host: the codes a client's
 * Base64::encode(cnn.gradients()) puts in the header slots (network.h:1038-1056: the block
 * counts and sizes) when `values` are those counts and sizes. FLEET_ERR_ARG: n < 0, or a
 * NULL array with n > 0. */
int fleet_gate_header_codes(const float* values, int n, int32_t* codes);
/* header_codes: one code per header position of the pool, in position order, or NULL: no
 * header check, and FLEET_ERRBIT_LAYOUT is never set. FLEET_ERR_ARG: a NULL pool or out;
 * codes given and n_headers other than the pool's header count. */
int fleet_gate_create(fleet_pool* pool, const int32_t* header_codes, int n_headers, fleet_gate** out);
void fleet_gate_destroy(fleet_gate* gate);
/* Vets the uploads in slots[0..K): the launches (fleet_acc_burst() slots each, the slots in
 * the kernel arguments) on the context's stream, one synchronisation, and status[k],
 * sumsq[k], max_abs[k] for slot slots[k]. FLEET_OK whenever the pass ran: a bad upload is a
 * result, not a failure of the call. FLEET_ERR_ARG, before anything is launched and with
 * the outputs untouched: K <= 0, a NULL argument, a slot outside [0, slots), an unoccupied
 * slot, a slot named twice. Waits for device puts in flight, as the pool's host forms do. */
int fleet_gate_vet(fleet_gate* gate, const int32_t* slots, int K, int32_t* status, double* sumsq, float* max_abs);
/* The same on the caller's stream into device arrays of K entries (int32, double, float),
 * without synchronisation; `slots` is still a host array. The gate's launch buffers are in
 * use until the stream has run the call: a later call of the pool or the gate on another
 * stream waits for it, as for a device put. */
int fleet_gate_vet_device(fleet_gate* gate, const int32_t* slots, int K, void* d_status, void* d_sumsq,
                          void* d_max_abs, void* stream);
/* One arrival, vetted on the request that brought it: fleet_pool_put's ingress into a FREE
 * slot (an occupied slot is FLEET_ERR_ARG; the other argument checks are fleet_pool_put's),
 * then the vet of that slot; synchronous. With a zero status the slot is occupied and the
 * call returns FLEET_OK. Otherwise the slot stays free -- the pool is as it was -- and the
 * call returns FLEET_ERR_BASE64 or FLEET_ERR_LAYOUT, BASE64 first, with the three outputs
 * filled. */
int fleet_gate_put(fleet_gate* gate, int slot, const char* upload, size_t len, int32_t* status, double* sumsq,
                   float* max_abs);

/* Kardam ledger: Kardam's `grads` map kept in HBM beside an upload pool --------
 * Kardam's bookkeeping runs in the staleSize > 0 branch alone (kardam.setModel /
 * setGrad / updateLip under modelsSize() == staleSize, CppNNUpdater.java:472-481),
 * the branch the pool covers. A fleet_kledger is Kardam.java's `grads` (worker ->
 * (g, epoch), Kardam.java:40, 56-71) with every g as one fp32 row in HBM, in upload
 * coordinates with header slots 0 (fleet_update_kardam_device's g_out rows). An
 * update through the ledger is fleet_pool_update plus setGrad for its picks, in pick
 * order: the fold kernel (k_pool_fold_kd) takes each pick's dampened value p on its
 * way into the sum and computes G = Q(f32(f64(p) * lr)) -- pickedGrad.scalarMultiply(
 * getLrate()), CppNNUpdater.java:478 --, its squared norm, the squared norm of
 * Q(G - prev) (g.subtract(prev).getNorm(), Kardam.java:63) and stores G, so the
 * picked rows are read once for the merged bytes and the side outputs together.
 *
 * A ledger belongs to one pool (same context, mutex and device; destroy it before
 * fleet_pool_destroy) whose window must cover the whole upload (a windowed pool is
 * FLEET_ERR_ARG: the norms are sums over all elements). It owns a slab of
 * workers + max_store fp32 rows of 12 G bytes rounded up to 16 (G groups), the
 * worker -> row and worker -> epoch tables and a free list of rows on the host, one
 * launch's per-wave norm partials (grid x 4 waves x fleet_acc_burst() picks x 2
 * doubles) and the pool's slots x 2 sums in HBM and pinned. `max_store` >= 1 bounds
 * the picks of one update that store a row. */
typedef struct fleet_kledger fleet_kledger;
int fleet_kledger_create(fleet_pool* pool, int workers, int max_store, fleet_kledger** out);
void fleet_kledger_destroy(fleet_kledger* ledger);
int fleet_kledger_workers(const fleet_kledger* ledger);
/* grads.containsKey(worker) (Kardam.java:57): 1 / 0; FLEET_ERR_ARG for NULL or a worker
 * outside [0, workers). */
int fleet_kledger_has(const fleet_kledger* ledger, int worker);
/* grads.get(worker).y (Kardam.java:59): the epoch recorded with the worker's row;
 * FLEET_ERR_ARG for NULL arguments, a worker outside [0, workers) or one not in the
 * ledger (*epoch untouched). */
int fleet_kledger_epoch(const fleet_kledger* ledger, int worker, int* epoch);
/* grads.remove(worker): the worker's row returns to the free list. FLEET_ERR_ARG as
 * fleet_kledger_epoch. */
int fleet_kledger_forget(fleet_kledger* ledger, int worker);
/* grads.get(worker).x decoded (Kardam.java:89-91): the worker's row, n = fleet_b64_count(
 * len) floats in upload coordinates, header slots 0. Synchronous. FLEET_ERR_ARG as
 * fleet_kledger_epoch; cap < n is FLEET_ERR_CAPACITY. */
int fleet_kledger_read(fleet_kledger* ledger, int worker, float* g, size_t cap);
/* fleet_pool_update* (CppNNUpdater.java:420-421, 463-464, 490-508) plus, for pick k of
 * worker[k] at model epoch epoch[k], kardam.setGrad(worker[k], pickedGrad.scalarMultiply(
 * lr), epoch[k]) (CppNNUpdater.java:478, Kardam.java:56-71), resolved on the host in pick
 * order before the launch:
 *   worker[k] < 0 (modelsSize()-1-tau < 0 or the modelsSize() == staleSize gate closed,
 *     CppNNUpdater.java:472-474, 483-484): set 0, norm_g and norm_diff NaN, nothing stored;
 *   not in the ledger (Kardam.java:67-70): set 0, norm_diff NaN, G stored;
 *   in the ledger with epoch[k] (Kardam.java:59-62, the push is ignored): set 0,
 *     norm_diff NaN, nothing stored;
 *   in the ledger with another epoch (Kardam.java:63-65): set 1, norm_diff =
 *     getNorm(g.subtract(prev)), G stored.
 * norm_g[k] = sqrt(sum (double)(G*G)) is g.getNorm() (Kardam.java:58), norm_diff
 * likewise over D = Q(G - prev): getNorm's float products summed in double in another
 * order (per wave, then the waves in a fixed order: no floating-point atomics, the same
 * bits for the same inputs on the same device). A worker that appears again later in the
 * same update sees what the earlier pick left: its prev is that pick's G, its epoch that
 * pick's. merged, merged_f32 and the slot status are fleet_pool_update's, bit for bit.
 *
 * Transactional: G goes to a free row, and worker -> row, the epoch and the free list
 * change only after the slot status was read back clean. On FLEET_ERR_BASE64 /
 * FLEET_ERR_LAYOUT the ledger (has, epoch, every row fleet_kledger_read returns) and the
 * pool are exactly as before, fleet_pool_slot_status names the slots, and the outputs
 * are not meaningful. FLEET_ERR_ARG, before anything is launched and with every output
 * untouched: everything fleet_pool_update rejects, a NULL worker, epoch, norm_g,
 * norm_diff or set, a worker >= workers, more storing picks than max_store, a
 * non-finite lr. Both forms synchronise once (the norms are host outputs); neither is
 * for graph capture. The device form uses fleet_pool_update_device's addressing. */
int fleet_kledger_update(fleet_kledger* ledger, const int32_t* picks, int K, const double* dampen,
                         const int32_t* worker, const int32_t* epoch, double lr, char* merged, size_t cap,
                         size_t* out_len, float* merged_f32, double* norm_g, double* norm_diff, uint8_t* set);
int fleet_kledger_update_device(fleet_kledger* ledger, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, void* stream);

/* Kardam Byzantine filter: what checkByz reads of an update's picks -------------
 * With the `true ||` of CppNNUpdater.java:488 removed a pick enters `avg` only if
 *   modelsSize() < staleSize || kardam.checkByz(id, pickedGrad, lastGrad, currModel, lastModel, tau)
 * and checkByz (Kardam.java:136-185) compares checkNorm -- getNorm(pickedGrad) /
 * getNorm(currModel) while lastGrad == null, else getNorm(pickedGrad.subtract(lastGrad)) /
 * getNorm(currModel.subtract(lastModel)) -- with a percentile of the workers' Lipschitz
 * coefficients. pickedGrad is the pick's dampened flat gradient p before the learning rate,
 * lastGrad the `avg` of the last update that had one (:510), currModel
 * getModelParametersNative(modelsSize()-1) at the start of the update (:417), lastModel the
 * currModel of the last update that had an `avg` (:511). None of the norms depends on a
 * decision of the same update, so one pass over the picks (k_pool_fold_kf, the filter form
 * of the ledger's fold) gives every pick's two norms beside everything fleet_kledger_update
 * gives, the host decides (percentile, counters: scalars), and fleet_kfilter_resolve folds
 * what was accepted.
 *
 * A filter belongs to one ledger (same pool, context, mutex and device; destroy it before
 * fleet_kledger_destroy). It owns lastGrad as two fp32 rows in upload coordinates -- one
 * read by the update, one that receives the avg of its result as lastGrad.subtract decodes
 * it, Q(f32(f64(sum) / accepted)) per flat slot (decodeFloat(merged) is that value decoded
 * and encoded once more, and differs from it where Q is not idempotent); they swap when a
 * resolve ends with an average --, one row of merged bytes and one of their fp32, two model rows of n =
 * n_biases * graph_edges + n_weights floats (current and last, fleet_mledger's row format),
 * and four sums per pick where the ledger has two. FLEET_ERR_ARG from create: NULLs,
 * graph_edges < 0, n = 0 or n >= 2^31 - 4096. */
typedef struct fleet_kfilter fleet_kfilter;
int fleet_kfilter_create(fleet_kledger* ledger, size_t n_weights, size_t n_biases, int graph_edges,
                         fleet_kfilter** out);
void fleet_kfilter_destroy(fleet_kfilter* filter);
/* lastGrad != null (Kardam.java:157): 1 / 0; FLEET_ERR_ARG for NULL. */
int fleet_kfilter_has_last(const fleet_kfilter* filter);
/* currModel = getModelParametersNative(modelsSize()-1) (CppNNUpdater.java:417) from the
 * vectors fleet_mledger_stage(_device) takes: the row a[i] = Q(param(i)), *norm_model =
 * getNorm(currModel) (Kardam.java:158) and, when a last model exists, *norm_model_diff =
 * getNorm(currModel.subtract(lastModel)) (:161), else NaN. Synchronous (the norms are host
 * outputs). The staged row becomes lastModel when the next resolve ends with an average
 * (:511); staging again before that replaces it. */
int fleet_kfilter_set_model(fleet_kfilter* filter, const float* weights, const float* biases, double* norm_model,
                            double* norm_model_diff);
int fleet_kfilter_set_model_device(fleet_kfilter* filter, const float* d_weights, const float* d_biases,
                                   double* norm_model, double* norm_model_diff, void* stream);
/* fleet_kledger_update(_device) plus, for every pick k (worker[k] < 0 included: the filter's
 * norm does not depend on the Kardam gate), norm_p[k] = getNorm(pickedGrad) (Kardam.java:158)
 * and norm_pdiff[k] = getNorm(pickedGrad.subtract(lastGrad)) (:160; E = Q(p - L) per flat
 * slot), NaN while there is no lastGrad. merged, merged_f32, norm_g, norm_diff, set, the slot
 * status, the ledger's rows and tables and every error with its transactional guarantee are
 * fleet_kledger_update's, bit for bit; on an error the filter's lastGrad and models are as
 * before too. The pass is optimistic: the outputs are the result with every pick accepted.
 * After FLEET_OK the update is pending until fleet_kfilter_resolve; until then the caller
 * must not fleet_pool_put(_device) into or fleet_pool_drop a picked slot. A new
 * fleet_kfilter_update discards a pending one (so does a failed one). Not for graph capture. */
int fleet_kfilter_update(fleet_kfilter* filter, const int32_t* picks, int K, const double* dampen,
                         const int32_t* worker, const int32_t* epoch, double lr, char* merged, size_t cap,
                         size_t* out_len, float* merged_f32, double* norm_g, double* norm_diff, uint8_t* set,
                         double* norm_p, double* norm_pdiff);
int fleet_kfilter_update_device(fleet_kfilter* filter, const int32_t* picks, int K, const double* dampen,
                                const int32_t* worker, const int32_t* epoch, double lr, void* d_merged,
                                void* d_merged_f32, double* norm_g, double* norm_diff, uint8_t* set, double* norm_p,
                                double* norm_pdiff, void* stream);
/* The pending update's result for the decisions accept[k] != 0 of its K picks
 * (CppNNUpdater.java:488-508):
 *   all accepted: the optimistic result, no fold is launched;
 *   a proper subset: avg over the accepted picks in pick order (the pool's fold without its
 *     finish, then the finish with inv = 1 / accepted) merged into the LAST of the K picks'
 *     upload, accepted or not (:508, pickedG), which overwrites the outputs;
 *   none: no average (:506), *out_len = 0, no output written.
 * With an average *out_len is the upload's length, lastGrad becomes this result's avg
 * (:510) and the model staged since the last resolve becomes lastModel (:511);
 * without one both stay. The update is then no longer pending. FLEET_ERR_ARG with
 * everything untouched (the update stays pending): a NULL filter, accept, merged or
 * out_len, no pending update, K other than the pending update's, a picked slot that is no
 * longer occupied. FLEET_ERR_CAPACITY as fleet_pool_update. Synchronous; not for graph
 * capture. The device form uses fleet_pool_update_device's addressing. */
int fleet_kfilter_resolve(fleet_kfilter* filter, const uint8_t* accept, int K, char* merged, size_t cap,
                          size_t* out_len, float* merged_f32);
int fleet_kfilter_resolve_device(fleet_kfilter* filter, const uint8_t* accept, int K, void* d_merged,
                                 void* d_merged_f32, size_t* out_len, void* stream);

/* Kardam model ledger: Kardam's `models` map kept in HBM -----------------------
 * kardam.setModel(pickedId, pickedModel) (CppNNUpdater.java:472-476) with pickedModel =
 * T_v = getModelParametersNative(v) (cppNN_backend.cpp:227-242: Base64::encode of
 * getModelParams, n = n_biases * graph_edges + n_weights values, fleet_model_params'
 * vector) is, per pick (Kardam.java:114-125):
 *   if models.containsKey(w):
 *     norm = mcurr.subtract(models.get(w)).getNorm()          (:117)
 *     if norm == 0: return                                     (:118-121, nothing changes)
 *     modelDiffNorm.put(w, norm)                               (:122)
 *   models.put(w, mcurr)                                       (:124)
 * and per element (cppNN_backend.cpp:779-795, 848-892), with Q = decodeFloat o encode:
 *   a = Q(P_v[i]), b = Q(P_u[i]), D = Q(a - b), norm = sqrt(sum (double)(D * D)).
 * A fleet_mledger keeps model VERSIONS as fp32 rows a[] in HBM (what decoding T_v gives:
 * Q applied once, never again; no text is built) under caller-chosen 64-bit ids, and
 * `models` as a worker -> row table with a reference count per row: storing a worker's
 * model copies nothing, and workers at one version share its row. The slab has workers +
 * max_versions rows of n floats rounded up to 4. Staging a version that is not resident
 * first evicts unreferenced rows, the one staged longest ago first, while there are
 * max_versions of them (staging a resident version renews its age); a row a worker holds
 * is never evicted. One update computes the norms of all distinct ordered (cur, prev) row
 * pairs its picks may need in launches of fleet_acc_burst() pairs (k_mrow_pair_norms); the
 * subtraction is not symmetric, the rule is "norm == 0" and not "same id", and a NaN norm
 * stores. Same context, mutex and device as `ctx`; destroy it before fleet_destroy.
 * FLEET_ERR_ARG from create: NULLs, workers or max_versions < 1, graph_edges < 0, n = 0 or
 * n >= 2^31 - 4096. */
typedef struct fleet_mledger fleet_mledger;
int fleet_mledger_create(fleet_ctx* ctx, size_t n_weights, size_t n_biases, int graph_edges, int workers,
                         int max_versions, fleet_mledger** out);
void fleet_mledger_destroy(fleet_mledger* ledger);
/* the sizes given to create; any pointer may be NULL */
int fleet_mledger_shape(const fleet_mledger* ledger, size_t* n_weights, size_t* n_biases, int* graph_edges,
                        int* workers, int* max_versions);
/* the context the ledger was made on (NULL for NULL) */
fleet_ctx* fleet_ctx_of_mledger(const fleet_mledger* ledger);
/* the pair kernel's launch shape, for tests and sizing: lanes per wave, values a block
 * takes per pass, blocks per pair at most (a lane strides on beyond values * blocks) */
int fleet_mledger_launch_shape(int* wave, int* block_values, int* max_blocks);
/* Make version `id` resident from its weights and use_bias() biases (fleet_model_export's
 * vectors): one pass (k_mrow_stage) writes a[i] = Q(param(i)) in getModelParams' order
 * (network.h:708-723, the biases repeated per layer-graph edge) and the row's own
 * getNorm (mcurr.getNorm(), Kardam.java:116). A resident id is a no-op (its content is not
 * compared; its age is renewed). The host form synchronises; the device form runs on
 * `stream`, and the ledger's later work is ordered after it. */
int fleet_mledger_stage(fleet_mledger* ledger, int64_t id, const float* weights, const float* biases);
int fleet_mledger_stage_device(fleet_mledger* ledger, int64_t id, const float* d_weights, const float* d_biases,
                               void* stream);
/* 1 / 0; FLEET_ERR_ARG for NULL */
int fleet_mledger_resident(const fleet_mledger* ledger, int64_t id);
/* setModel for K picks in pick order (CppNNUpdater.java:476, Kardam.java:114-125): pick k
 * is version id[k] for worker[k]; worker[k] < 0 = Kardam does not run for that pick
 * (CppNNUpdater.java:472-474, 483-484; id[k] is not looked at). status[k]:
 *   0 skipped; 1 first model for that worker (stored, norm_diff NaN); 2 ignored (norm ==
 *   0: nothing changes, norm_diff 0); 3 set (stored, norm_diff = the norm, NaN included).
 * norm_model[k] = getNorm(T_v) (NaN for a skipped pick). A worker picked again later in
 * the same update sees what its earlier pick left. The norms are getNorm's float products
 * summed in double in another order (per wave, the waves and blocks in a fixed order: no
 * floating-point atomics, the same bits for the same inputs on the same device); a norm
 * that is exactly 0 in the reference is exactly 0 here.
 * FLEET_ERR_ARG, before anything is launched and with every output and the ledger
 * untouched: NULLs, K < 0, a worker >= workers, an id that is not resident, more distinct
 * picked versions that no worker holds than max_versions. K = 0 or all workers < 0
 * launches nothing. Synchronises once (the norms are host outputs); not for graph capture. */
int fleet_mledger_update(fleet_mledger* ledger, const int64_t* id, const int32_t* worker, int K,
                         double* norm_model, double* norm_diff, uint8_t* status);
/* models.containsKey(worker) (Kardam.java:115): 1 / 0; FLEET_ERR_ARG for NULL or a worker
 * outside [0, workers). */
int fleet_mledger_has(const fleet_mledger* ledger, int worker);
/* the id of the version models.get(worker) is; FLEET_ERR_ARG as fleet_mledger_has, or for
 * a worker without a model (*id untouched) */
int fleet_mledger_version(const fleet_mledger* ledger, int worker, int64_t* id);
/* models.remove(worker): the row loses a reference (and stays resident until evicted).
 * FLEET_ERR_ARG as fleet_mledger_version. */
int fleet_mledger_forget(fleet_mledger* ledger, int worker);
/* decodeFloat(models.get(worker)): the n values of the worker's row. Synchronous.
 * FLEET_ERR_ARG as fleet_mledger_version; cap < n is FLEET_ERR_CAPACITY. */
int fleet_mledger_read(fleet_mledger* ledger, int worker, float* params, size_t cap);
/* the same for a resident version by id */
int fleet_mledger_read_version(fleet_mledger* ledger, int64_t id, float* params, size_t cap);

/* Self-test of the device codec arithmetic over whole input domains: an
 * order-independent 64-bit digest sum_i splitmix64(i<<32 | f(i)) of
 *   fn 0: int2float over all 2^32 codes      fn 1: float2int over all 2^32 bit patterns
 *   fn 2: Q fast path over |x| < 1           fn 3: int2float fast path (codes % 10 == 0)
 *   fn 4: t/10 (div10) for 1e-30 <= t < inf  fn 5: packed Q fast path
 *   fn 6: variable-length Q (-1e8 < x < 1e9)  fn 7: variable-length int2float (all codes)
 *   fn 8: packed fn 6 on (x, -x/4)            fn 9: packed fn 7 on (c, c*2654435761)
 *   fn 10: variable-length float2int (-1e8 < x < 1e9)   fn 11: float2int fast path (|x| < 1)
 *   fn 12: select-chain Q of the serial accumulation (-1e8 < x < 1e9; same digest as fn 6)
 *   fn 13: multiplier-table Q (as fn 6)   fn 14: multiplier-table int2float (as fn 7)
 *   fn 15: multiplier-table float2int (as fn 10)   fn 16: scalar Q fast path (as fn 2)
 *   fn 17: one-lookup latency Q (q_xl) on |x| < 1e8, fn 12 elsewhere (as fn 6)
 *   fn 18: the teacher forward's expf (glibc 2.35 restated) over all 2^32 inputs,
 *          NaN results as 0x7fc00000 (the libm expf digest of tests/native/digest_ref.cpp)
 *   fn 19: byte-table Q of the stream kernel (q_d16 + compare fix-up; as fn 6)
 *   fn 20: byte-table float2int of the client encode (enc_d16; as fn 10)
 *   fn 21: the serial accumulation's Q with VarEntry digit offsets (var_d16; as fn 6)
 *   fn 22: the model-version copy's strtof("%.6g") round trip over every finite
 *          binary32 (decimal6.h; against libc's snprintf/strtof)
 *   fn 23: the stream kernels' int2float (dec_d16; as fn 0)
 *   fn 24: the text of `ostream << float` (decimal6.h g6_text) over all 2^32 bit
 *          patterns: sum_i g6_text_term(i, text) against libc's snprintf("%g")
 *          (tests/native/check_g6text.cpp, tests/golden/g6text_digest.json)
 *   fn 25..28: the solvers' arithmetic (solver_math.h, x86 NaN rule applied) against
 *          tests/native/check_solver.cpp on the CPU (tests/golden/solver_digests.json):
 *          fn 25 sqrtf(x), fn 26 adam's denominator (float)sqrt((double)x / (1. - .999f)) +
 *          1e-8f, fn 27 x / (1.f - .9f), each over all 2^32 x with fn 0's term; fn 28 a / b
 *          over 2^32 pairs (a, b) = (low, high word of splitmix64(i)) and every pair of
 *          {+-0, the smallest and largest denormal, FLT_MIN, 1, FLT_MAX, +-inf, +-NaN},
 *          term splitmix64(splitmix64(a << 32 | b) + bits(a / b));
 *          fn 29, 30 = fn 26, 27 with a server session's b2_t = .999f*.999f, b1_t = .9f*.9f
 * computed on the GPU; compare with the oracle's digests. */
int fleet_selftest_digest(fleet_ctx* ctx, int fn, uint64_t* out);

/* DISTILLATION_MODE=1 model codec -- host buffers ----
 * `weights` = the model's W matrices concatenated in W order, `dims` =
 * n_mats x {cols, rows, chans} (W matrices are not channel-aligned: each is
 * cols*rows*chans floats). */
/* network::quantization_weight_model (commonLib/cppNN/network.h:1683-1774,
 * core_math.h:881-912) on a copy of the weights, then getParams' first-occurrence
 * dictionary (float_vector_find, network.h:594-608, |a-b| < 1e-8f) and the
 * selected-index set (network.h:641-692). Outputs, each nullable: quantized[n]
 * (the weights the text describes), dict[n] (entries in creation order, *n_dict
 * of them), index[n] (the printed index; -1 for NaN/inf weights). */
int fleet_model_quantize_index(fleet_ctx* ctx, const float* weights, const int32_t* dims, int n_mats,
                               float* quantized, float* dict, int* n_dict, int32_t* index);
/* The DISTILLATION_MODE=1 weights section of getParams (network.h:641-692) for
 * these weights: "n\nU\n", U pairs "k\nvalue\n" (value as `ostream << float`,
 * i.e. %g), one line of "index " per matrix -- the bytes the reference emits
 * after the bias lines (getParametersNative, Server/.../cppNN_backend.cpp:244-280). */
int fleet_model_weights_text(fleet_ctx* ctx, const float* weights, const int32_t* dims, int n_mats, char* out,
                             size_t cap, size_t* out_len);
/* The text of `ostream << float` (default precision: snprintf("%g")) for n
 * values, every byte formatted on the device (decimal6.h g6_text: the exact six
 * digits from integer arithmetic; 0, -0, inf, -inf, nan, -nan for the rest).
 *   n_blocks > 0: block_sizes[n_blocks] sums to n; "value " per value and '\n'
 *     after each block -- the bias lines and DISTILLATION_MODE=0 weight lines of
 *     getParams (network.h:611-706). A block of size 0 prints its lone '\n';
 *     at most 254 empty blocks may follow one another.
 *   n_blocks == 0: "i\nvalue\n" for i = 0..n-1, the mode-1 dictionary section.
 * n < 2^31. *out_len is set even when cap is too small (FLEET_ERR_CAPACITY).
 * The _device form reads the values where they are (no host to device copy). */
int fleet_values_text(fleet_ctx* ctx, const float* values, size_t n, const int64_t* block_sizes, int n_blocks,
                      char* out, size_t cap, size_t* out_len);
int fleet_values_text_device(fleet_ctx* ctx, const void* d_values, size_t n, const int64_t* block_sizes, int n_blocks,
                             char* out, size_t cap, size_t* out_len, void* stream);
/* network::read's DISTILLATION_MODE=1 weights branch (network.h:958-997): such a
 * section back to weights (W[i] = value of the index's dictionary key; a key
 * the dictionary lacks gives 0.0f, std::map::operator[]). */
int fleet_model_read_weights(fleet_ctx* ctx, const char* text, size_t len, const int32_t* dims, int n_mats,
                             float* weights_out);

/* descentNative's DISTILLATION_MODE=1 model copy (Server/src/main/c++/
 * cppNN_backend.cpp:355-372: cnnNew->read(cnn.getParams()) of the unquantised
 * model, network.h:611-706 + 956-997): every weight becomes the %g/strtof
 * round trip of its first-occurrence dictionary entry (|a-b| < 1e-8f), every
 * bias the round trip of itself. The O(n*U) dictionary scans of the reference
 * become a device sort, and the decimal round trips run on the device too
 * (exact integer arithmetic, checked against libc's snprintf/strtof on every
 * finite binary32). Non-finite weights or biases: FLEET_ERR_ARG (the
 * reference's text parse fails on "nan"/"inf"). */
int fleet_model_version(fleet_ctx* ctx, const float* weights, const int32_t* dims, int n_mats, const float* biases,
                        size_t n_biases, float* weights_out, float* biases_out);

/* getModelParametersNative (Server/src/main/c++/cppNN_backend.cpp:227-242, SURVEY.md
 * §8 a20): Base64::encode of network::getModelParams (commonLib/cppNN/network.h:
 * 708-723) = the biases of every use_bias() layer (layer order) repeated
 * graph_edges = layer_graph.size() times -- the bias loop sits inside the loop
 * over layer_graph -- then the non-null W. Output: fleet_b64_len(n_biases *
 * graph_edges + n_weights) bytes. */
int fleet_model_params_device(fleet_ctx* ctx, const float* d_weights, size_t n_weights, const float* d_biases,
                              size_t n_biases, int graph_edges, void* d_out, void* stream);
int fleet_model_params(fleet_ctx* ctx, const float* weights, size_t n_weights, const float* biases, size_t n_biases,
                       int graph_edges, char* out, size_t cap, size_t* out_len);

/* getMiniBatch (Server/src/main/c++/cppNN_backend.cpp:677-699):
 * Base64::encode of the vector uniformSample / nonIIDSample build (:553-675) --
 * header[7] = {E, sigma, C, lr, batchSize, featureSize, numLabels} as float (the
 * caller converts as push_back does), then per sample idx[b] its F features,
 * (DISTILLATION_MODE=1, teacher != NULL) the teacher's num_labels probabilities
 * teacher[b*num_labels ..], and its label as float; with a teacher the vector
 * ends with 1234567 (:611). The index draw (rand() % N, or the non-IID bucket
 * cursor) stays with the caller (fleet_amd/sampler.py mirrors both); the
 * teacher's forward pass is not rebuilt (its outputs are inputs).
 * images: n_images x F fp32 rows; labels: n_images int32. Output:
 * fleet_minibatch_len(F, B, num_labels, teacher != NULL) bytes. */
size_t fleet_minibatch_len(int F, int B, int num_labels, int with_teacher);

/* The sampler's mode-1 teacher forward: uniformSample appends
 * teacher.forward(sample, TEMPERATURE, -1, 1)'s 10 class probabilities per drawn
 * sample (Server/src/main/c++/cppNN_backend.cpp:596-613) for the teacher network
 * initSampler builds (:494-502: I1 28x28, C1 conv 5x5x8 elu, P1 semi-stochastic
 * pool 3, C2i conv 1x1x16 elu, C2 conv 5x5x48 elu, P2 semi-stochastic pool 2,
 * FC2 softmax 10), computed as commonLib/cppNN's network::forward does, bit for
 * bit (expf = glibc 2.35's, fleet_amd/csrc/teacher_math.h). w: the network's
 * non-null W in order (fleet_teacher_weight_count() floats), b: the use_bias()
 * layers' biases in layer order (fleet_teacher_bias_count()); the first 784 of
 * each image's F features are the input; temperature = TEMPERATURE (2,
 * commonLib/cppNN/network.h:53). Replaces the teacher.forward calls; the
 * teacher's training in initSampler stays with the caller. */
size_t fleet_teacher_weight_count(void);
size_t fleet_teacher_bias_count(void);
/* device buffers: probs[b*10 + j] for image d_idx[b] (d_idx NULL: image b);
 * an index outside [0, n_images) is reported by fleet_check as FLEET_ERR_ARG */
int fleet_teacher_forward_device(fleet_ctx* ctx, const void* d_w, const void* d_b, const void* d_images,
                                 size_t n_images, int F, const void* d_idx, int B, float temperature, void* d_probs,
                                 void* stream);
/* host buffers, synchronous: probs[B x 10] for images[idx[b]] */
int fleet_teacher_forward(fleet_ctx* ctx, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* idx, int B, float temperature, float* probs);

/* Evaluation: the Driver's test() (Driver/src/main/c++/cppNN_backend.cpp:53-75, called by
 * evaluateNative :201-205 on the network of :109-115, the teacher's network above), bit for
 * bit. For image k of the B evaluated, in the order given:
 *   out  = cnn.forward(x_k, 1.f, thread, 0) (commonLib/cppNN/network.h:523-592): the
 *          teacher's forward at temperature 1 with both semi-stochastic pools at
 *          train == 0 (commonLib/cppNN/layer.h:540: the largest value always);
 *   argm = arg_max(out, 10) (network.h:146-153; predict_class :510-515): ties keep the
 *          first index, a NaN never wins and never loses its place;
 *   p = out[argm]; cost_k = ((0.5f * d) * d), d = p - (float)label_k (cost.h:49-51: the
 *          target is the label itself); correct += (argm == label_k);
 * then error = (0.f + cost_0 + cost_1 + ...) / (float)B, added in binary32 in image order,
 * and accuracy = ((float)correct / (float)B) * 100.f. Without NaN among weights, biases
 * and pixels every output is bit-identical to the reference's; with NaN inputs the NaN
 * positions and every other value are, NaN bit patterns are not pinned.
 * B <= 0 is FLEET_ERR_ARG (the reference divides 0 by 0).
 * w / b: fleet_teacher_forward's layout; images [n_images][F], F >= 784 (the first 784
 * floats of a row are read); labels [n_images] int32; idx NULL (images 0..B-1, B <=
 * n_images) or B indices into the images. */
/* images a block of the forward kernel takes at a time (its group size) */
size_t fleet_evaluate_block_images(void);
/* tests: cap the forward kernel's grid at max_blocks so that a small B walks more than one
 * grid-stride pass (0: the default, three blocks per CU); returns the previous cap */
int fleet_evaluate_set_grid(int max_blocks);
/* device buffers, on the caller's stream, not synchronised. Per-image outputs d_pred
 * (int32[B]), d_prob (float[B], p), d_cost (float[B]), d_probs10 (float[B][10]) may each
 * be NULL; d_result: float error, float accuracy, int32 correct. Costs and predictions
 * the caller does not take go to a workspace of the context, allocated on first use and
 * grown only for a larger B; evaluations that use it must be ordered with each other (one
 * stream, or d_cost and d_pred of the caller's own). An index outside [0, n_images) is
 * reported by fleet_check as FLEET_ERR_ARG, the outputs then unspecified. */
int fleet_evaluate_device(fleet_ctx* ctx, const void* d_w, const void* d_b, const void* d_images, size_t n_images, int F,
                          const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob, void* d_cost,
                          void* d_probs10, void* d_result, void* stream);
/* host buffers, synchronous; error, accuracy, correct, pred[B] and prob[B] may each be
 * NULL. FLEET_ERR_ARG before any launch: NULL inputs, F < 784, B <= 0, n_w / n_b other than
 * fleet_teacher_weight_count() / fleet_teacher_bias_count(), an index outside the images. */
int fleet_evaluate(fleet_ctx* ctx, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                   size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B, float* error,
                   float* accuracy, int32_t* correct, int32_t* pred, float* prob);

/* The same test() (Driver/src/main/c++/cppNN_backend.cpp:53-75) on the reference's CIFAR
 * network (:128-138), bit for bit, `classes` = 10 or 100 (:136, :135):
 *   I1 input 32 32 3, C1 convolution 3 16 1 elu, P1 max_pool 3 2, C2 convolution 3 64 1 elu,
 *   P2 max_pool 4 4, local4 fully_connected 384 relu, local5 fully_connected 192 relu,
 *   FC2 fully_connected `classes` softmax.
 * Per image cnn.forward(x, 1.f, thread, 0) (commonLib/cppNN/network.h:523-592): the
 * convolutions of layer.h:805-872 in the non-AVX order of core_math.h:136-148, 172-185 (one
 * running binary32 sum per output, input channel outer, nine taps inner) with elu::fc
 * (activation.h:172-179); max_pool (layer.h:363-456: strict `<`, ties keep the first, a NaN
 * in first place stays); fully_connected (layer.h:200-239, dot of core_math.h:67-70) with
 * relu::f (activation.h:199-206) and, for FC2, softmax::f at temperature 1 (:273-286); then
 * arg_max, the cost and the closing lines as fleet_evaluate states them, under the same NaN
 * rule. fleet_amd/csrc/cifar_forward.h restates the arithmetic.
 * w: the non-null W in order, C1 432, C2 9216, local4 221184, local5 73728, FC2 192 *
 * classes; b: the use_bias() layers' biases in layer order, 16, 64, 384, 192, classes
 * (FC2's are carried and not read: softmax adds none). images [n_images][F], F >= 3072:
 * the first 3072 floats of a row are read, planar (channel, row, column), as
 * commonLib/cppNN/cifar_parser.h:88-94 delivers them. */
/* the vector lengths for classes 10 (306480, 666) and 100 (323760, 756); 0 for any other */
size_t fleet_cifar_weight_count(int classes);
size_t fleet_cifar_bias_count(int classes);
/* images a block of the forward kernel takes at a time (its group size) */
size_t fleet_cifar_block_images(void);
/* tests: cap the forward kernel's grid at max_blocks so that a small B walks more than one
 * grid-stride pass (0: the default, one block per CU); returns the previous cap */
int fleet_cifar_set_grid(int max_blocks);
/* device buffers, on the caller's stream, not synchronised. Per-image outputs d_pred
 * (int32[B]), d_prob (float[B], p), d_cost (float[B]), d_probsN (float[B][classes]) may each
 * be NULL; d_result: float error, float accuracy, int32 correct. Costs and predictions the
 * caller does not take go to fleet_evaluate_device's workspace, under its rule: allocated on
 * first use, grown only for a larger B (the old one retired, not freed), and calls that use
 * it ordered with each other. An index outside [0, n_images) is reported by fleet_check as
 * FLEET_ERR_ARG, the outputs then unspecified. FLEET_ERR_ARG at once: NULL inputs, classes
 * not 10 or 100, F < 3072, B <= 0, B > n_images without indices. */
int fleet_cifar_test_device(fleet_ctx* ctx, int classes, const void* d_w, const void* d_b, const void* d_images,
                            size_t n_images, int F, const void* d_labels, const void* d_idx, int B, void* d_pred,
                            void* d_prob, void* d_cost, void* d_probsN, void* d_result, void* stream);
/* host buffers, synchronous; error, accuracy, correct, pred[B], prob[B], cost[B] and
 * probsN[B][classes] may each be NULL. FLEET_ERR_ARG before any launch: NULL inputs, classes
 * not 10 or 100, F < 3072, B <= 0, n_w / n_b other than fleet_cifar_weight_count(classes) /
 * fleet_cifar_bias_count(classes), an index outside the images. */
int fleet_cifar_test(fleet_ctx* ctx, int classes, const float* w, size_t n_w, const float* b, size_t n_b,
                     const float* images, size_t n_images, int F, const int32_t* labels, const int32_t* idx, int B,
                     float* error, float* accuracy, int32_t* correct, int32_t* pred, float* prob, float* cost,
                     float* probsN);

/* The client's gradients: Java_..._getGradients' hot loop (Client/app/src/main/cpp/
 * cppNN-lib.cpp:101-113 the train_class calls, :218-234 cnn.gradients() and the upload), for
 * C clients of B samples each. Client c's row is the float vector cnn.gradients() returns
 * (commonLib/cppNN/network.h:1038-1056, after sync_mini_batch :1289-1331) once train_class
 * (:1806-2008, with backward_hidden :1551-1611) has run on its B samples in the single-thread
 * order, sample k taking batch slot k, on the MNIST network above with the cross_entropy
 * cost: fleet_client_grad_len() = 22961 values, [nW, (size, dW..)*, nB, (size, dbias..)*].
 * Per sample: m.shift(dx, dy, mojo::edge) (:1840), forward(input, temperature, thread, 1)
 * (the client passes a teacher_prob, so TEMPERATURE = 2; 1 without), the output delta
 * 1.f * (node - target) with a one-hot target (all zeros for a label outside [0, 10)), both
 * passes of backward_hidden in the reference's order of operations (fleet_amd/csrc/
 * client_backward.h restates it), then dW_sets[0] += dW_sets[b] in sample order. Bit-identical
 * to the reference whenever no intermediate is NaN. A sample whose E is NaN (the reference
 * bails) is reported by fleet_check as FLEET_ERR_ARG, its client's row then unspecified; with a
 * NaN met only in the backward pass, NaN positions and bit patterns are not pinned.
 * DPgradients and the distillation cost: the _ex_ forms below. Not covered: the client's own
 * descent, the reference's thread race. */
size_t fleet_client_grad_len(void);
/* tests: walk the clients in chunks of at most max_clients (0: the default, what fits a
 * 256 MiB workspace of per-sample rows); returns the previous value */
int fleet_client_grad_set_chunk(int max_clients);
/* device buffers, on the caller's stream, not synchronised. d_models: n_models rows of
 * model_pitch floats, each w then b in fleet_teacher_forward's layout; d_model_of_client:
 * int32[C] row per client, or NULL for row 0. d_images [n_images][F] (F >= 784), d_labels
 * int32[n_images]; d_idx int32[C][B], or NULL for images c*B + k; d_shift int32[C][B][2]
 * = {dx, dy} each in {-1, 0, 1}, or NULL for no shift. d_grads: C rows of grad_pitch floats
 * (>= 22961). d_uploads: NULL, or C rows of upload_pitch bytes (a multiple of 16, >=
 * 16 * ceil(22961 / 3)) that receive Base64::encode of the rows, the text fleet_update_device
 * and fleet_pool_put_device take. The per-sample rows go to a workspace of the context,
 * allocated on first use and grown only for a larger need; calls that use it must be ordered
 * with each other. An image index, a model row or a shift outside its range is reported by
 * fleet_check as FLEET_ERR_ARG, the outputs then unspecified. */
int fleet_client_grads_device(fleet_ctx* ctx, const void* d_models, size_t model_pitch, int n_models,
                              const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                              const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                              float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                              size_t upload_pitch, void* stream);
/* host buffers, one model for every client, synchronous. grads [C][22961]; uploads NULL or C
 * rows of upload_pitch bytes (>= fleet_b64_len(22961)). FLEET_ERR_ARG before any launch: NULL
 * inputs, F < 784, C <= 0, B <= 0, n_w / n_b other than fleet_teacher_weight_count() /
 * fleet_teacher_bias_count(), an index outside the images, a shift outside {-1, 0, 1}. */
int fleet_client_grads(fleet_ctx* ctx, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                       size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts, int C,
                       int B, float temperature, float* grads, char* uploads, size_t upload_pitch);

/* The two other configurations of getGradients: the distillation cost and DPgradients.
 * (The names carry `_ex_` in the middle; the argument lists are those of fleet_client_grads,
 * fleet_client_grads_device and fleet_rmodel_client_grads_device with cost, clip and sigma
 * after temperature.)
 * cost: FLEET_COST_CROSS_ENTROPY, or FLEET_COST_DISTILLATION for start_epoch("distillation")
 * (cppNN-lib.cpp:251-252 under DISTILLATION_MODE 1): the output delta is
 * distillation::d_cost(node, target, teacher, T) * softmax::df(node, j, 10, T)
 * (commonLib/cppNN/network.h:1959, cost.h:93-113, activation.h:301-304) with T = temperature;
 * d_cost never reads the teacher's value, so no soft labels are taken. E stays the mean of
 * mse::cost.
 * clip, sigma: host float[C], both NULL for no DP, else both given. Client c with sigma[c] > 0
 * gets what cnn.DPgradients(clip[c], sigma[c]) returns (cppNN-lib.cpp:218-219, 295-296;
 * network.h:1092-1181): scale_gradients over batch slots 1 .. B-1 (sqsum in binary32 in the
 * reference's walk, layers last to first, each layer's dW block then its dbias block;
 * scale = 1 / max(1, sqrt(sqsum) / clip); slot 0 is never clipped; as written there only the
 * dbias blocks are multiplied by scale, no dW is: both kept), the ordered sum, then
 * addGaussian(C * sigma) (:1125-1130) on every slot and the sizes written back over the header
 * slots. The draws are fleet_client_dp_noise's, the same on every call, as the reference
 * default-constructs its engine on every call. A client with sigma[c] == 0 gets
 * cnn.gradients(), exactly the rows of the calls above. The arrays are copied to the device
 * on the call's stream before the launches (pageable source: the copy has left them when the
 * call returns).
 * FLEET_ERR_ARG before any launch, besides the refusals of the calls above: an unknown cost;
 * one of clip / sigma NULL and the other not; a negative or non-finite sigma; with sigma > 0,
 * a clip that is <= 0 or non-finite. */
#define FLEET_COST_CROSS_ENTROPY 0
#define FLEET_COST_DISTILLATION 1
/* fleet_client_grads_device (cppNN-lib.cpp:101-113, 218-234, 251-252; network.h:1092-1181) */
int fleet_client_ex_grads_device(fleet_ctx* ctx, const void* d_models, size_t model_pitch, int n_models,
                                 const void* d_model_of_client, const void* d_images, size_t n_images, int F,
                                 const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                                 float temperature, int cost, const float* clip, const float* sigma, void* d_grads,
                                 size_t grad_pitch, void* d_uploads, size_t upload_pitch, void* stream);
/* fleet_client_grads (cppNN-lib.cpp:101-113, 218-234, 251-252; network.h:1092-1181) */
int fleet_client_ex_grads(fleet_ctx* ctx, const float* w, size_t n_w, const float* b, size_t n_b, const float* images,
                          size_t n_images, int F, const int32_t* labels, const int32_t* idx, const int32_t* shifts,
                          int C, int B, float temperature, int cost, const float* clip, const float* sigma,
                          float* grads, char* uploads, size_t upload_pitch);
/* host only: the first n (<= 22961) of the standard-normal draws addGaussian adds, before they
 * are scaled by C * sigma (network.h:1125-1130): std::normal_distribution<double>(0.0, 1.0) on
 * a default-constructed std::default_random_engine, from the C++ library this one is built
 * with, as the reference client's come from its own. The library makes the table once, on
 * the first DP call, on the host; a context uploads it on its own first DP call and keeps it
 * resident. Nothing of it is computed on the device. */
int fleet_client_dp_noise(double* out, size_t n);

/* Kardam bookkeeping of CppNNUpdater.update (Server/src/main/java/apps/cppNN/
 * CppNNUpdater.java:463-481, utils/Kardam.java:48-62) for the M
 * picked uploads in one call:
 *   g_c = ByteVec(getFlatGradient(upload_c)).scalarMultiply(dampen_c).scalarMultiply(lr)
 * (flat Base64, the text Kardam.setGrad stores), norm_g[c] = g_c.getNorm() and,
 * when prev[c] != NULL (the worker's previous g, same length),
 * norm_diff[c] = g_c.subtract(prev[c]).getNorm(), else NaN. The uploads share
 * the last one's layout (as fleet_update enforces). g_out: M rows of g_pitch
 * bytes (>= *g_len). Norms: partial sums of the reference's fp64 loop in a
 * different order (1e-12 relative). */
int fleet_kardam_grads(fleet_ctx* ctx, const char* const* uploads, const size_t* lens, int M, const double* dampen,
                       double lr, const char* const* prev, char* g_out, size_t g_pitch, size_t* g_len,
                       double* norm_g, double* norm_diff);
/* device-resident dataset, indices (d_idx[B]) and output; an index outside
 * [0, n_images) is reported by fleet_check as FLEET_ERR_ARG */
int fleet_minibatch_device(fleet_ctx* ctx, const void* d_images, size_t n_images, int F, const void* d_labels,
                           const void* d_idx, int B, const void* d_teacher, int num_labels, const float header[7],
                           void* d_out, void* stream);
/* host buffers: the B sampled rows are gathered into pinned staging, encoded on
 * the GPU and returned (synchronous); FLEET_ERR_ARG for an index outside the set */
int fleet_minibatch(fleet_ctx* ctx, const float* images, size_t n_images, int F, const int32_t* labels,
                    const int32_t* idx, int B, const float* teacher, int num_labels, const float header[7],
                    char* out, size_t cap, size_t* out_len);

/* descentNative's model step -------------------------------
 * Server/src/main/c++/cppNN_backend.cpp:336-352: network::descent(vector)
 * (commonLib/cppNN/network.h:1185-1202) walks the gradients() layout of the
 * merged gradient -- w_sizes[n_w] weight blocks, b_sizes[n_b] bias blocks -- and
 * descent() (:1334-1353) applies
 *   sgd::increment_w (solver.h:88-94):  w -= lr*(dW + 0*w)   per weight block i
 *                                         with w_present[i] (W[i] non-null)
 *   update_bias (layer.h:241-243):       b -= db*lr           per layer k with
 *                                         fc_layer[k] (fully_connected_layer)
 * in fp32, one rounding per operation. `weights` = the non-null W concatenated in
 * slot order (the model codec's layout); `fc_bias` = the fully-connected layers'
 * biases concatenated in layer order; `grad` = decodeFloat(merged) (fleet_update's
 * merged_f32), n_up floats. lr = (float)lrates_vec[currEpoch].
 * Device-resident (layout arrays on the host; the header values inside d_grad
 * are not re-read: fleet_update already checked them against the layout). */
int fleet_descent_device(fleet_ctx* ctx, float* d_weights, float* d_fc_bias, const float* d_grad,
                         const int32_t* w_sizes, const uint8_t* w_present, int n_w, const int32_t* b_sizes,
                         const uint8_t* fc_layer, int n_b, float lr, void* stream);
/* The same model step on one element shard (fleet_amd.shard): d_grad_window holds
 * the merged fp32 values [value_begin, value_end) of the upload positions (what
 * fleet_update_device's window mode writes); only the weights and FC biases whose
 * gradient positions fall in the window are updated, in the full-size model
 * arrays -- so N ranks, each on its window, update disjoint parts with no
 * exchange, and together do exactly fleet_descent_device's step. */
int fleet_descent_window_device(fleet_ctx* ctx, float* d_weights, float* d_fc_bias, const float* d_grad_window,
                                size_t value_begin, size_t value_end, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream);
/* Host buffers, updated in place; checks the header floats of grad against the
 * layout as network::descent(vector) would read them (FLEET_ERR_LAYOUT). */
int fleet_descent(fleet_ctx* ctx, float* weights, size_t n_weights, float* fc_bias, size_t n_fc_bias,
                  const float* grad, size_t n_grad, const int32_t* w_sizes, const uint8_t* w_present, int n_w,
                  const int32_t* b_sizes, const uint8_t* fc_layer, int n_b, float lr);

/* The model step under the reference's other solvers ---------
 * `mojo::network cnn(solver.c_str())` (cppNN_backend.cpp:40-42) runs the named
 * solver's increment_w in network::descent() (commonLib/cppNN/solver.h:97-195):
 *   adagrad  g1 += d*d;                       w -= (lr*d) / (sqrt(g1) + 1e-8f)
 *   rmsprop  g1 = .999f*g1 + ((1-.999f)*d)*d; w -= (lr*d) / (sqrt(g1) + 1e-8f), lr = .01f*L
 *   adam     g1 = .9f*g1 + (1-.9f)*d; g2 = .999f*g2 + ((1-.999f)*d)*d;          lr = .1f*L
 *            w -= (lr*(g1/(1.f-.9f))) / ((float)sqrt((double)g2/(1.-.999f)) + 1e-8f)
 * one IEEE rounding per operation in the type shown (solver_math.h). adam's .9f and
 * .999f in the last line are its b1_t and b2_t, which adam::reset multiplies by b1 and
 * b2: the two entry points below use a fresh solver's values, as written above; the
 * models use a server session's (see fleet_model_set_solver). The state g1 (and g2, adam) is one
 * float per weight, laid out like `weights`, zero before the first step, advanced
 * in place; biases step by update_bias with the plain L whatever the solver. */
#define FLEET_SOLVER_SGD 0
#define FLEET_SOLVER_ADAGRAD 1
#define FLEET_SOLVER_RMSPROP 2
#define FLEET_SOLVER_ADAM 3
/* new_solver's names ("sgd", "adagrad", "rmsprop", "adam"); -1 for any other, NULL included */
int fleet_solver_from_name(const char* name);
/* fleet_descent_device under `solver`. g1 / g2: n_weights floats each on the device;
 * g2 may be NULL unless solver is adam, g1 may be NULL for sgd (FLEET_ERR_ARG
 * otherwise, and for an unknown solver). FLEET_SOLVER_SGD is fleet_descent_device's
 * step exactly. */
int fleet_descent_solver_device(fleet_ctx* ctx, int solver, float* d_weights, float* d_g1, float* d_g2,
                                float* d_fc_bias, const float* d_grad, const int32_t* w_sizes,
                                const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer,
                                int n_b, float lr, void* stream);
/* fleet_descent under `solver`: host buffers updated in place, the same header check */
int fleet_descent_solver(fleet_ctx* ctx, int solver, float* weights, size_t n_weights, float* g1, float* g2,
                         float* fc_bias, size_t n_fc_bias, const float* grad, size_t n_grad, const int32_t* w_sizes,
                         const uint8_t* w_present, int n_w, const int32_t* b_sizes, const uint8_t* fc_layer, int n_b,
                         float lr);

/* The server's resident model -----------------------
 * The state the reference's updater natives keep in libnative.so globals
 * (Server/src/main/c++/cppNN_backend.cpp: cnn, models, lrates_vec, currEpoch,
 * priority), built on the entry points above. Errors: fleet_model_last_error.
 * distillation_mode = the reference's compile-time DISTILLATION_MODE (1: the
 * quantised dictionary / index-set text; 0: plain values). */
typedef struct fleet_model fleet_model;
/* fetchParamsNative (:282-301): network::read of a getParams text (mojo01 format,
 * commonLib/cppNN/network.h:611-706, 840-1010). Layer types: input,
 * convolution, max_pool, semi_stochastic_pool, fully_connected (FLeet's cppNN
 * models); W shapes follow the layers' new_connection rules (layer.h). */
int fleet_model_load(fleet_ctx* ctx, const char* text, size_t len, int distillation_mode, fleet_model** out);
void fleet_model_destroy(fleet_model* m);
const char* fleet_model_last_error(const fleet_model* m);
/* initUpdater's model part (:161-194): lr = (float)lrates[0], the first version
 * (read(getParams()) of the model) pushed, priority = epoch = 0. */
int fleet_model_init_updater(fleet_model* m, const double* lrates, int n_lrates);
/* descentNative (:329-383): decodeFloat(merged); lr = lrates[epoch] while epoch <
 * n_lrates; network::descent (sgd w -= lr*dW, fully-connected biases b -= db*lr,
 * fleet_descent); epoch++; the new version read(getParams()) appended and the
 * oldest dropped beyond stale_size. The merged gradient's header must describe
 * the model (FLEET_ERR_LAYOUT otherwise; the reference overruns). */
int fleet_model_descent(fleet_model* m, const char* merged, size_t len, int client_batch_size, int stale_size);
/* The solver `cnn` is constructed with (new_solver's names; the default is "sgd"). To be
 * called after load and before the first descent: it allocates the zeroed state, which
 * belongs to cnn alone (versions carry none, getParams prints none). FLEET_ERR_ARG for an
 * unknown name (the reference dereferences NULL there) and after a descent, with
 * nothing changed. A refused gradient leaves the state as it was; the mode-1
 * non-finite-weight case leaves it advanced, as it leaves cnn.
 * adam in a session: fetchParamsNative's start_epoch resets the solver once
 * (network.h:1442; before the model is read, so no state is cleared), which leaves
 * b1_t = .9f*.9f and b2_t = .999f*.999f for every descent of the session; nothing decays
 * them further. adagrad's state starts at zero like the others' (the reference leaves
 * it as the heap gave it: its fill(0) is commented out, solver.h:105-107). */
int fleet_model_set_solver(fleet_model* m, const char* name);
int fleet_model_solver(fleet_model* m); /* FLEET_SOLVER_* */
/* state row `which` (0: g1, 1: g2) of n_weights floats; FLEET_ERR_ARG for a row the
 * solver does not keep, FLEET_ERR_CAPACITY for cap < n_weights */
int fleet_model_solver_state(fleet_model* m, int which, float* out, size_t cap);
/* modelsSize (:324-327) */
int fleet_model_count(fleet_model* m);
/* getParametersNative(version) (:244-280): the full getParams text of
 * models[version] -- header, bias lines (ostream precision 6), weights
 * (mode 1: quantization_weight_model's dictionary and index set, the version
 * itself left unquantised). */
int fleet_model_get_params(fleet_model* m, int version, char* out, size_t cap, size_t* out_len);
/* getModelParametersNative(version) (:227-242): Base64 of getModelParams. */
int fleet_model_get_model_params(fleet_model* m, int version, char* out, size_t cap, size_t* out_len);
/* getCurrEpoch/setCurrEpoch, getPriority/setPriority, getLrate (:129-159) */
int fleet_model_get_epoch(fleet_model* m);
void fleet_model_set_epoch(fleet_model* m, int epoch);
int fleet_model_get_priority(fleet_model* m);
void fleet_model_set_priority(fleet_model* m, int priority);
double fleet_model_get_lrate(fleet_model* m);
/* sizes: non-null W floats, use_bias() biases, layer-graph edges, layers */
int fleet_model_shape(fleet_model* m, size_t* n_weights, size_t* n_biases, int* graph_edges, int* n_layers);
/* weights / biases of models[version] (version -1: the current `cnn`) */
int fleet_model_export(fleet_model* m, int version, float* weights, size_t n_weights, float* biases, size_t n_biases);
/* A stable id of models[version]: the count of versions pushed before it (initUpdater's
 * is 0). Indices into `models` shift when descentNative drops the oldest (:369-371); the
 * id of a version never changes. FLEET_ERR_ARG for NULLs or a version outside models. */
int fleet_model_version_id(fleet_model* m, int version, int64_t* id);
/* fleet_mledger_stage of models[version] under its fleet_model_version_id (written to *id
 * when not NULL): what kardam.setModel is given at CppNNUpdater.java:473-476, without the
 * text. FLEET_ERR_ARG when the ledger's n_weights, n_biases or graph_edges differ from
 * fleet_model_shape's, or as fleet_model_version_id. */
int fleet_mledger_stage_model(fleet_mledger* ledger, fleet_model* m, int version, int64_t* id);
/* fleet_evaluate of models[version] (version -1: cnn), whose vectors are uploaded as the
 * model's other natives upload theirs: what Evaluator.crossValidation gets from
 * fetchParamsNative + evaluateNative (Driver/src/main/c++/cppNN_backend.cpp:179-205) of
 * that version's text. The model must be the MNIST network of :109-115 -- I1 input 28 28 1,
 * C1 convolution 5 8 1 elu, P1 semi_stochastic_pool 3 3, C2i convolution 1 16 1 elu, C2
 * convolution 5 48 1 elu, P2 semi_stochastic_pool 2 2, FC2 fully_connected 10 softmax --
 * or FLEET_ERR_ARG names the first layer that differs, with nothing launched. */
int fleet_model_evaluate(fleet_model* m, int version, const float* images, size_t n_images, int F,
                         const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                         int32_t* correct, int32_t* pred, float* prob);
/* fleet_cifar_test of models[version] (version -1: cnn), as fleet_model_evaluate is
 * fleet_evaluate of it: fetchParamsNative + evaluateNative (Driver/src/main/c++/
 * cppNN_backend.cpp:179-205) of that version's text on the CIFAR network of :128-138. The
 * model must be that network -- I1 input 32 32 3, C1 convolution 3 16 1 elu, P1 max_pool 3 2,
 * C2 convolution 3 64 1 elu, P2 max_pool 4 4, local4 fully_connected 384 relu, local5
 * fully_connected 192 relu, FC2 fully_connected 10 or 100 softmax, from which `classes` is
 * read -- or FLEET_ERR_ARG names the first layer that differs, with nothing launched. */
int fleet_model_cifar_test(fleet_model* m, int version, const float* images, size_t n_images, int F,
                           const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                           int32_t* correct, int32_t* pred, float* prob);

/* The same model resident in HBM (fleet_rmodel): `cnn` and every entry of `models`
 * live on the device, so a model step takes a merged gradient that is already there
 * (fleet_update_device / fleet_pool_update_device / fleet_kledger_update_device's
 * d_merged_f32) and leaves the new version where the Kardam model ledger stages it
 * device to device; only texts leave the device. Same natives, same results bit for
 * bit as fleet_model (the yardstick). Errors: fleet_rmodel_last_error.
 *
 * HBM: (max_versions + 2) rows of [weights | use_bias() biases], 64 floats aligned
 * (cnn and a ring of max_versions + 1 versions: descentNative pushes before it pops),
 * plus a workspace allocated once at load (the dictionary pipeline's buffers and
 * rocPRIM storage, the text emitters', the text and a20 buffers; fleet_rmodel_
 * workspace_bytes). After load only the staging of a host gradient text grows, on the
 * first fleet_rmodel_descent (and for a longer text); fleet_rmodel_stats counts every
 * hipMalloc / hipHostMalloc made. Guarded by a mutex; every entry restores the
 * caller's device. max_versions >= 1.
 * Streams: the _device entry points (fleet_rmodel_descent_device,
 * fleet_rmodel_get_model_params_device) run on the stream they are given, NULL
 * meaning the null stream as in the rest of this C-ABI, so they order with the
 * work that wrote their inputs and with the caller's next use of their outputs
 * on that stream. fleet_rmodel_descent_device synchronises it (the error word);
 * fleet_rmodel_get_model_params_device does not, and its version must not be
 * dropped before the stream has passed it. The host-buffer entry points run on a
 * stream of the model's own and return synchronised. */
typedef struct fleet_rmodel fleet_rmodel;
int fleet_rmodel_load(fleet_ctx* ctx, const char* text, size_t len, int distillation_mode, int max_versions,
                      fleet_rmodel** out);
void fleet_rmodel_destroy(fleet_rmodel* m);
const char* fleet_rmodel_last_error(const fleet_rmodel* m);
int fleet_rmodel_init_updater(fleet_rmodel* m, const double* lrates, int n_lrates);
/* descentNative from the merged text: decoded on the device; fleet_model_descent's
 * header checks and errors (FLEET_ERR_BASE64, FLEET_ERR_LAYOUT, FLEET_ERR_ARG), made
 * by a check kernel before any weight is written: a refused gradient changes nothing.
 * A step after which more than max_versions versions would be kept (stale_size larger
 * than the model was loaded for) is refused with FLEET_ERR_ARG before anything
 * changes. DISTILLATION_MODE=1 with a non-finite weight or bias after the step:
 * FLEET_ERR_ARG with cnn stepped, the epoch advanced and no version pushed, as
 * fleet_model_descent leaves its model. */
int fleet_rmodel_descent(fleet_rmodel* m, const char* merged, size_t len, int client_batch_size, int stale_size);
/* The same from decodeFloat of the merged text on the device (n_values floats).
 * n_values below the model's shortest gradient (2 + graph edges + layers + weights +
 * fc biases) is FLEET_ERR_ARG with nothing launched; the exact length follows from the
 * gradient's own bias-block sizes and is checked with the header slots on the device.
 * Synchronous: one 4-byte error word is read back per step. */
int fleet_rmodel_descent_device(fleet_rmodel* m, const void* d_merged_f32, size_t n_values, int stale_size,
                                void* stream);
/* fleet_model_set_solver / _solver / _solver_state on the resident model: the state rows
 * are n_weights floats each in HBM, allocated zeroed by the call and counted in
 * fleet_rmodel_stats; the check kernel refuses a gradient before any weight or state
 * float is written. */
int fleet_rmodel_set_solver(fleet_rmodel* m, const char* name);
int fleet_rmodel_solver(fleet_rmodel* m);
int fleet_rmodel_solver_state(fleet_rmodel* m, int which, float* out, size_t cap);
int fleet_rmodel_count(fleet_rmodel* m);
/* getParametersNative: the header is constant; the bias lines, the mode-0 weight lines,
 * the mode-1 dictionary lines and the index section are formatted on the device from
 * the resident row into one buffer and copied out once. No weight travels host to
 * device. fleet_rmodel_params_cap: a capacity that always suffices. */
size_t fleet_rmodel_params_cap(const fleet_rmodel* m);
int fleet_rmodel_get_params(fleet_rmodel* m, int version, char* out, size_t cap, size_t* out_len);
int fleet_rmodel_get_model_params(fleet_rmodel* m, int version, char* out, size_t cap, size_t* out_len);
/* the a20 text into a device buffer of fleet_b64_len(n_biases * graph_edges + n_weights)
 * bytes rounded up to 16, plus 16 (fleet_model_params_device's kernel, on `stream`) */
int fleet_rmodel_get_model_params_device(fleet_rmodel* m, int version, void* d_out, void* stream);
int fleet_rmodel_get_epoch(fleet_rmodel* m);
void fleet_rmodel_set_epoch(fleet_rmodel* m, int epoch);
int fleet_rmodel_get_priority(fleet_rmodel* m);
void fleet_rmodel_set_priority(fleet_rmodel* m, int priority);
double fleet_rmodel_get_lrate(fleet_rmodel* m);
int fleet_rmodel_shape(fleet_rmodel* m, size_t* n_weights, size_t* n_biases, int* graph_edges, int* n_layers);
int fleet_rmodel_export(fleet_rmodel* m, int version, float* weights, size_t n_weights, float* biases,
                        size_t n_biases);
int fleet_rmodel_version_id(fleet_rmodel* m, int version, int64_t* id);
/* models[version]'s weights and biases where they live (version -1: cnn); valid until
 * that version is dropped */
int fleet_rmodel_version_device(fleet_rmodel* m, int version, const float** d_weights, const float** d_biases);
/* fleet_mledger_stage_model from the resident row, device to device, same ids; FLEET_ERR_ARG
 * for a ledger of another context than the model's */
int fleet_rmodel_stage_mledger(fleet_mledger* ledger, fleet_rmodel* m, int version, int64_t* id);
/* resident_bytes: the rows, 4 * roundup64(n_weights + n_biases) * (max_versions + 2), plus
 * 4 * n_weights per state row of the solver (fleet_rmodel_set_solver);
 * device_allocs: every hipMalloc / hipHostMalloc made on the model's behalf so far */
int fleet_rmodel_stats(fleet_rmodel* m, size_t* resident_bytes, int* device_allocs);
size_t fleet_rmodel_workspace_bytes(const fleet_rmodel* m);
/* fleet_model_evaluate of the resident row (fleet_rmodel_version_device's pointers): no
 * weight crosses PCIe. The device form takes images, labels and indices where they live,
 * runs on the caller's stream and does not synchronise (an index outside the images:
 * fleet_check of the model's context); d_pred / d_prob may be NULL. The host form uploads
 * images, labels and indices and returns synchronised. The B costs and predictions the
 * caller does not take, and the host form's staging, come from a workspace allocated on
 * first use, grown only for a larger need and counted in fleet_rmodel_stats; a model's
 * evaluations must be ordered with each other (they share it). */
int fleet_rmodel_evaluate_device(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F,
                                 const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob,
                                 void* d_result, void* stream);
int fleet_rmodel_evaluate(fleet_rmodel* m, int version, const float* images, size_t n_images, int F,
                          const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                          int32_t* correct, int32_t* pred, float* prob);
/* fleet_model_cifar_test of the resident row, in fleet_rmodel_evaluate's two forms and under
 * its rules (Driver/src/main/c++/cppNN_backend.cpp:53-75, 128-138, 179-205): no weight crosses
 * PCIe, the device form runs on the caller's stream and does not synchronise, the workspace is
 * the evaluation's (one allocation serves both, counted in fleet_rmodel_stats). F >= 3072. */
int fleet_rmodel_cifar_test_device(fleet_rmodel* m, int version, const void* d_images, size_t n_images, int F,
                                   const void* d_labels, const void* d_idx, int B, void* d_pred, void* d_prob,
                                   void* d_result, void* stream);
int fleet_rmodel_cifar_test(fleet_rmodel* m, int version, const float* images, size_t n_images, int F,
                            const int32_t* labels, const int32_t* idx, int B, float* error, float* accuracy,
                            int32_t* correct, int32_t* pred, float* prob);
/* fleet_client_grads_device with the models taken from the resident rows where they live
 * (cppNN-lib.cpp:101-113, 218-234; network.h:1806-2008, 1551-1611, 1289-1331, 1038-1056):
 * versions[C] (host) names client c's model as fleet_rmodel_evaluate_device names a version
 * (-1: cnn); a client on an older version is FLeet's staleness. The MNIST network only. Runs
 * on the caller's stream and does not synchronise (fleet_check of the model's context). */
int fleet_rmodel_client_grads_device(fleet_rmodel* m, const int32_t* versions, const void* d_images, size_t n_images,
                                     int F, const void* d_labels, const void* d_idx, const void* d_shift, int C, int B,
                                     float temperature, void* d_grads, size_t grad_pitch, void* d_uploads,
                                     size_t upload_pitch, void* stream);
/* fleet_rmodel_client_grads_device with the cost and the DP parameters of
 * fleet_client_ex_grads_device (cppNN-lib.cpp:218-221, 251-252; network.h:1092-1181) */
int fleet_rmodel_client_ex_grads_device(fleet_rmodel* m, const int32_t* versions, const void* d_images, size_t n_images,
                                        int F, const void* d_labels, const void* d_idx, const void* d_shift, int C,
                                        int B, float temperature, int cost, const float* clip, const float* sigma,
                                        void* d_grads, size_t grad_pitch, void* d_uploads, size_t upload_pitch,
                                        void* stream);

/* The offline sampler's state (the CppNNOfflineSampler natives
 * of Server/src/main/c++/cppNN_backend.cpp and the globals they keep). Random
 * draws come from libc rand(), the process-wide generator the reference uses.
 * Errors: fleet_sampler_last_error. */
typedef struct fleet_sampler fleet_sampler;
/* initSampler (:385-479): srand(seed) (the reference's seed is 1, :71), the
 * MNIST training set under data_path (commonLib/cppNN/mnist_parser.h:
 * train-images.idx3-ubyte or train-images-idx3-ubyte and the labels file,
 * pixels (b / 255) * 2 - 1), numLabels = 10, and with iid == 0 the non-IID
 * buckets (:411-479): sort_indexes of the labels (std::sort), with outlier != 0
 * a first bucket of the label-0 samples, then 2*(num_clients - outliers) shards
 * shuffled and dealt two per client, every bucket shuffled (std::random_shuffle
 * over rand() % i). iid, outlier and num_clients are the reference's
 * compile-time globals (:59-61; defaults 0, 0, 10). The teacher's training that
 * follows in DISTILLATION_MODE=1 whatever the sampler (:481-545) is not rebuilt:
 * iid mini-batches take the trained weights from fleet_sampler_set_teacher.
 * ctx may be NULL (host state only; fleet_sampler_minibatch then fails). */
int fleet_sampler_create(fleet_ctx* ctx, const char* data_path, int iid, int outlier, int num_clients,
                         int distillation_mode, int seed, fleet_sampler** out);
/* the same over a dataset in memory: images n x F floats, labels n */
int fleet_sampler_create_from(fleet_ctx* ctx, const float* images, const int32_t* labels, size_t n, int F,
                              int num_labels, int iid, int outlier, int num_clients, int distillation_mode, int seed,
                              fleet_sampler** out);
void fleet_sampler_destroy(fleet_sampler* s);
const char* fleet_sampler_last_error(const fleet_sampler* s);
/* initUpdater's generator side effects (:163, :216/:222): srand(seed), then, when
 * a model was fetched (fetched != 0: fetchParamsNative's set_random_augmentation
 * enabled the random shift, :293), the two rand() draws of cnn.train_class's shift
 * (network.h:1840). Assumes the reference's MNIST network: no dropout layer (whose
 * training forward would draw more, layer.h:608-617) and no flips. */
void fleet_updater_reseed_ex(int seed, int fetched);
/* the original one-argument form: fleet_updater_reseed_ex(seed, 1) (a model was
 * fetched, the reference's server order) -- kept so callers built against it keep
 * their meaning */
void fleet_updater_reseed(int seed);
/* initUpdater's E, sigma, C (:169-171), read by every later mini-batch header */
int fleet_sampler_set_hyper(fleet_sampler* s, int E, double sigma, double C);
/* DISTILLATION_MODE=1 with iid sampling: the trained teacher's weights
 * (fleet_teacher_forward's layout); uniformSample then appends its outputs */
int fleet_sampler_set_teacher(fleet_sampler* s, const float* w, size_t n_w, const float* b, size_t n_b);
/* getMiniBatch (:677-699): B = batch_size * E samples -- uniformSample's
 * rand() % N draws, or nonIIDSample's cursor over the current client's bucket
 * -- the client rotation advanced, header {E, sigma, C, lr, B, F, numLabels}
 * (lr = the updater's cnn.get_learning_rate()), encoded on the GPU
 * (fleet_minibatch). B <= 0 (E = 0 before initUpdater) is FLEET_ERR_ARG: the
 * reference reads sample 0 of an empty batch there. */
int fleet_sampler_minibatch(fleet_sampler* s, int batch_size, float lr, char* out, size_t cap, size_t* out_len);
size_t fleet_sampler_minibatch_len(fleet_sampler* s, int batch_size);
int fleet_sampler_num_labels(const fleet_sampler* s);   /* getNumLabels (:129-132) */
int fleet_sampler_has_outlier(const fleet_sampler* s);  /* hasOutlier (:134-137) */
size_t fleet_sampler_num_samples(const fleet_sampler* s);
/* introspection (tests): bucket `client` (positions in the label-sorted order),
 * the label-sorted order itself, and the last request's image indices */
int fleet_sampler_bucket(fleet_sampler* s, int client, int32_t* out, size_t cap, size_t* n);
int fleet_sampler_sorted_index(fleet_sampler* s, int32_t* out, size_t cap, size_t* n);
int fleet_sampler_last_indices(fleet_sampler* s, int32_t* out, size_t cap, size_t* n);

/* Name of the aggregation kernel fleet_update / fleet_update_device launch for
 * an upload of `len` Base64 bytes (or a group window of that many bytes), exactly
 * as rocprofv3 names it (every template argument spelled out): "k_update_mixed<256,
 * false>", "k_update_flat", "k_update_weave<8>", "k_update_tiled_encode<64>" (tile=classic)
 * or "k_update_pipe<16, 1, 5, 0, false>"; and what fleet_update_encode_device launches
 * ("k_update_encode<256>", "k_update_tiled_encode<64>", "k_update_flat",
 * "k_update_weave_encode<8>", ...; DESIGN.md §4 lists the default per size;
 * profiling aid; thread-local storage, valid until the thread's next call). */
const char* fleet_update_kernel(size_t len);
const char* fleet_update_encode_kernel(size_t len);
/* The same plan's grid (test and profiling aid, no device needed): kind 0 stream
 * (blocks [0, n_a) a group per lane, 256 groups each, the rest a value per lane,
 * 84 groups each), 1 tiled (n_w 64-group tiles then n_n 16-group tiles; n_w = -1:
 * one width, 64-group tiles only), 2 pipelined (16-group tiles), 3 woven tiles
 * (64 groups each), 4 flat tiles (n_w 64-group tiles, then n_n tiles of n_a
 * groups, the last one ragged); *blocks = the aggregation's grid. */
int fleet_update_plan_grid(size_t len, int* kind, int64_t* blocks, int64_t* n_a, int64_t* n_w, int64_t* n_n);

/* Launch-plan overrides, process-wide (experiments, and tests that run every
 * launch variant on small inputs; results are identical under every plan). spec =
 * comma-separated key=value items: update=auto|stream|tiled|pipe, grid=auto|plain|balanced|
 * lanes (the stream grid; lanes = every group a value per lane, the balanced grid's tail
 * form, for tests on small inputs), tile=auto|classic|flat|weave6|weave8 and
 * flat_w2=auto|1..64, tile_enc_prio=auto|0..3 (the tiles' form; the flat grid's
 * narrow width; the tiles' fused encode blocks' issue priority), tile_enc_rows=N,
 * fused=on|off (the pipelined step as one launch or two), stage_threads=1..64,
 * stage_pieces=1..64 (host staging); ""
 * restores the measured default. An unknown key or value rejects the whole spec
 * (FLEET_ERR_ARG, the reason in err) and leaves the plan unchanged. The environment
 * variable FLEET_EXPERIMENTS, read once at first use, takes the same spec; no other
 * environment variable changes a launch. fleet_plan returns the active spec ("" =
 * default; thread-local storage). */
int fleet_set_plan(const char* spec, char* err, size_t cap);
const char* fleet_plan(void);

/* Test hook (no reference counterpart): the pipelined Kardam form's reduce blocks of
 * this context wait for the launch's epoch + skew, which no tile publishes when skew
 * != 0, so their bounded wait times out and fleet_update_kardam_device returns
 * FLEET_ERR_HIP. skew = 0 restores the normal hand-off. */
int fleet_test_kardam_skew(fleet_ctx* ctx, unsigned skew);

#ifdef __cplusplus
}
#endif
#endif
