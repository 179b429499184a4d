/*
 * trlda_hip.h -- C ABI of libtrlda_hip.so, the MI355X (gfx950) implementation of
 * trlda's per-document variational E-step and the lambda M-step around it.
 *
 * This is the drop-in boundary: plain pointers and sizes, status-code returns
 * (0 = ok, negative = error, message via trlda_last_error()), no exceptions and
 * no torch / Eigen / CPython types cross it.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repository).
 *
 * Conventions (identical to the reference's in-memory layout):
 *   - every matrix is column-major fp64 (Eigen default; python/src/pyutils.cpp:22-26):
 *       lambda, sstats : K x V, element (k, w) at [k + K*w]
 *       gamma          : K x B, element (k, d) at [k + K*d]
 *   - a batch of documents is CSR int32: indptr[B+1], ids[nnz], cnts[nnz]; this is
 *     the flat form of LDA::Documents = vector<vector<pair<int,int>>>
 *     (include/lda.h:21-23) that PyList_ToDocuments builds
 *     (python/src/ldainterface.cpp:152-190).  Duplicate ids inside a document and
 *     zero counts are legal.  Word ids are validated (0 <= id < V); the reference
 *     has undefined behaviour there.
 *   - "host" pointers are ordinary memory; "dev" pointers are HIP device
 *     addresses on the model's device (hipMalloc'ed by trlda_dev_alloc or by
 *     anyone else, e.g. a torch tensor's data_ptr()).
 *   - functions taking a trlda_model enqueue work on the model's stream and
 *     return without synchronising unless they copy to host memory.  That stream is a
 *     non-blocking stream of the model's own until trlda_model_set_stream hands it
 *     another one: it does NOT order itself against the legacy null stream, so device
 *     buffers a caller fills or reads on a stream of its own must either be complete
 *     (trlda_model_synchronize / trlda_dev_synchronize) or that stream be the model's.
 *
 * There is NO CPU fallback behind this header: with no usable GPU every compute
 * entry point returns TRLDA_ERR_NO_DEVICE.
 */
#ifndef TRLDA_HIP_H
#define TRLDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRLDA_OK               0
#define TRLDA_ERR_ARG         -1  /* bad argument (null pointer, negative size ...)       */
#define TRLDA_ERR_SHAPE       -2  /* TRLDA::Exception("... wrong dimensionality.")         */
#define TRLDA_ERR_WORD_ID     -3  /* word id outside [0, V)                                */
#define TRLDA_ERR_NO_DEVICE   -4  /* no HIP device / HIP runtime error at init             */
#define TRLDA_ERR_HIP         -5  /* a HIP call failed; see trlda_last_error()             */
#define TRLDA_ERR_VALUE       -6  /* TRLDA::Exception("... should not be negative.")       */

/* how sufficient statistics are accumulated (trlda_model_set_sstats_mode) */
#define TRLDA_SSTATS_SEGMENTED 0  /* per-word ordered sums via the batch's word-major index:
                                     bitwise reproducible, same addition order as the
                                     reference's serial loop (lda.cpp:207-213)              */
#define TRLDA_SSTATS_ATOMIC    1  /* fp64 global atomics from the document kernel           */

typedef struct trlda_model trlda_model;   /* device-resident lambda, alpha, workspaces */
typedef struct trlda_batch trlda_batch;   /* device-resident CSR batch + word-major index */

/* ---- library ---------------------------------------------------------- */

const char *trlda_last_error(void);       /* thread-local, never NULL */
int trlda_version(void);
int trlda_device_count(void);             /* number of HIP devices, 0 if none */

/* The largest number of topics the variational path (every entry point that runs a VI E-step:
 * the estep, stream, corpus, update, lower-bound and predictive calls, trlda_estep) takes: the
 * general document kernel keeps 3 K + 4 doubles per workgroup in LDS (160 KiB on gfx950).  Above
 * it those calls return TRLDA_ERR_ARG before they draw, copy or launch anything; Gibbs sampling,
 * top words and sampling documents have bounds of their own.  trlda_vi_check_topics(K): that
 * check on its own (TRLDA_OK, or TRLDA_ERR_ARG and the message). */
#define TRLDA_VI_MAX_TOPICS 6814
int trlda_vi_max_topics(void);
int trlda_vi_check_topics(int K);

/* ---- host-side RNG: bit-compatible with the reference ------------------ */

/* trlda.seed(): srand(seed).  python/src/module.cpp:332-342 */
void trlda_seed(unsigned int seed);

/* The state of that stream (33 words), so that the ranks of a data-parallel job can adopt
 * rank 0's: the reference has one process and one stream (src/lda.cpp:71, :135); replicas that
 * draw "the same" gamma0 must share it. */
void trlda_rng_get_state(uint32_t *state33);
void trlda_rng_set_state(const uint32_t *state33);

/* sampleGamma(m, n, k): -sum_{i<k} log|U_i|, U = -1 + 2*rand()/RAND_MAX, k passes over
 * an m x n column-major matrix, libc rand() consumed in exactly the reference's order.
 * src/utils.cpp:224-231, Eigen/src/Core/MathFunctions.h:439-446.  Host memory. */
void trlda_sample_gamma(int m, int n, int k, double *out);

/* sampleGamma(m, n, 100) / 100.: the lambda init of LDA::LDA (src/lda.cpp:71) and the
 * default gamma init of LDA::updateVariables (src/lda.cpp:135).  Host memory. */
void trlda_sample_gamma_init(int m, int n, double *out);

/* ---- one-shot, host pointers ------------------------------------------- */

/*
 * LDA::updateVariables(documents, latents, parameters) with inferenceMethod == VI:
 * include/lda.h:109-112 -> src/lda.cpp:142-156 -> LDA::updateVariablesVI,
 * src/lda.cpp:160-220.  Called by python/src/ldainterface.cpp:367-370
 * (update_variables / do_e_step).
 *   gamma     in: initial gamma (K x B);  out: gamma after inference
 *   sstats    out: K x V sufficient statistics (already multiplied by exp E[log beta])
 *   iters_out optional (may be NULL): fixed-point iterations executed per document
 *   device    HIP device ordinal
 * Uploads, runs the HIP kernels, downloads, synchronises.
 */
int trlda_estep(int K, int V, int B,
                const int32_t *indptr, const int32_t *ids, const int32_t *cnts,
                const double *lambda, const double *alpha,
                double *gamma, double *sstats,
                int max_iter, double threshold, int32_t *iters_out, int device);

/*
 * LDA::updateVariables(documents, latents, parameters) with inferenceMethod == GIBBS:
 * src/lda.cpp:142-156 -> LDA::updateVariablesGibbs, src/lda.cpp:224-293 (one-shot
 * trlda_model_gibbs_host; the drop-in boundary of INTEGRATION.md).
 *   theta        in (use_latents != 0): initial theta (K x B); out: sampled theta
 *   sstats       out: K x V statistics, 1 / num_samples per token and sample
 * Uploads, runs the HIP kernels, downloads, synchronises.
 */
int trlda_gibbs(int K, int V, int B,
                const int32_t *indptr, const int32_t *ids, const int32_t *cnts,
                const double *lambda, const double *alpha,
                double *theta, int use_latents, double *sstats,
                int num_samples, int burn_in, int device);

/* lambda = (1-rho) lambda' + rho (eta + scale * sstats): src/onlinelda.cpp:99-100 and
 * :108-109 (scale = D / B); src/batchlda.cpp:60 is the rho = 1, scale = 1 case. */
int trlda_mstep_blend(int K, int V, double rho, double eta, double scale,
                      const double *lambda_prime, const double *sstats,
                      double *lambda_out, int device);

/* Trust-region initial step, src/onlinelda.cpp:79-86:
 * lambda[:, w] = (1-rho) lambda'[:, w] + rho (eta + D/B/K * wordcounts[w]). */
int trlda_tr_init(int K, int V, int B, int num_documents, double rho, double eta,
                  const int32_t *indptr, const int32_t *ids, const int32_t *cnts,
                  const double *lambda_prime, double *lambda_out, int device);

/* ---- text corpora (host side) ---------------------------------------------------------
 *
 * The reference's corpus files (python/utils/load_documents.py:6-69): one document per line,
 * "<n> id:cnt id:cnt ...", the leading <n> ignored like line.split()[1:] does.  The file is
 * mapped and parsed by the library's host threads straight into CSR -- the form
 * trlda_batch_create takes: batch b of documents [d0, d1) is
 * indptr = offsets[d0 .. d1] - offsets[d0], ids + offsets[d0], cnts + offsets[d0].
 * Tokens that are not [+-]digits:[+-]digits within int32, and files with bare carriage
 * returns, fail with TRLDA_ERR_VALUE / TRLDA_ERR_ARG and a line number in trlda_last_error(). */
typedef struct trlda_docs trlda_docs;
int trlda_docs_from_text(const char *path, trlda_docs **out);
/* the same for text already in memory (a window of a file that does not fit: the Python loader
 * reads bounded chunks cut at line ends); `bytes` of `text`, the last line may lack its newline */
int trlda_docs_from_buffer(const char *text, size_t bytes, trlda_docs **out);
int64_t trlda_docs_num_docs(const trlda_docs *docs);
int64_t trlda_docs_nnz(const trlda_docs *docs);
const int64_t *trlda_docs_offsets(const trlda_docs *docs);   /* num_docs + 1 */
const int32_t *trlda_docs_ids(const trlda_docs *docs);       /* nnz */
const int32_t *trlda_docs_cnts(const trlda_docs *docs);      /* nnz */
int trlda_docs_destroy(trlda_docs *docs);

/* ---- device memory helpers (so a host program needs no HIP headers) ---- */

int trlda_dev_alloc(int device, size_t bytes, void **dev_out);
int trlda_dev_free(int device, void *dev);
int trlda_dev_upload(int device, void *dev_dst, const void *host_src, size_t bytes);
int trlda_dev_download(int device, void *host_dst, const void *dev_src, size_t bytes);
int trlda_dev_synchronize(int device);

/* ---- batches ------------------------------------------------------------ */

/* Validates (monotone indptr, 0 <= id < V), uploads the CSR arrays and builds the
 * word-major index (stable counting sort by word id) used by the segmented
 * sufficient-statistics kernel.  Replaces PyList_ToDocuments' deep copy
 * (python/src/ldainterface.cpp:152-190).
 *
 * On the caller's thread: the validation -- every error of the arguments is this call's -- and one
 * copy of the three arrays into pinned memory (they are the caller's again on return): ~8-12 us per
 * 200 documents instead of ~75.  The index (csrc/batch_index.cpp: host work only) is built on the
 * library's worker threads (TRLDA_INDEX_THREADS, default 4; 0: on this thread, as before round 6), up
 * to two dozen batches at a time.  The workers make NO HIP call: a finished index is uploaded --
 * an allocation, one copy on the library's upload stream (a 16-workgroup kernel that reads the pinned
 * buffer over PCIe; hipMemcpyAsync's call blocked for milliseconds now and then: TRLDA_UPLOAD_COPY=memcpy
 * for A/B), two events: ~10 us -- by a caller's thread,
 * whichever comes first: the next trlda_batch_create (which uploads what was finished since the last
 * one), the E-step the batch is announced to (`next`, `upcoming[]` below), or the batch's first user.
 * Every entry point that is handed the batch waits for the index -- or, when no worker has started on
 * it yet, does the work itself, so that "create, use at once" costs what it did.  A batch destroyed
 * before anybody used it is never indexed.  An index is there ~170 us after its trlda_batch_create
 * (a queue, 40 us in which a caller that uses its batch at once is left alone with it, ~80 us of work):
 * a stream makes its batches eight steps ahead of their use (bench.py, value_end_to_end).  A failed
 * upload (out of device memory) fails the batch's first use, with the build's status and message.
 * An announced batch whose index is not there yet counts as not announced.
 * (TRLDA_INDEX_UPLOAD=worker: the workers enqueue the uploads too, one at a time -- the first form of
 * round 6, kept for A/B: four threads in hipMemcpyAsync / hipEventRecord beside the caller's launches
 * spent 32-175 us per build in the runtime's locks.) */
int trlda_batch_create(trlda_batch **out, int device, int V, int B,
                       const int32_t *indptr, const int32_t *ids, const int32_t *cnts);
int trlda_batch_destroy(trlda_batch *batch);
int trlda_batch_num_docs(const trlda_batch *batch);
int64_t trlda_batch_nnz(const trlda_batch *batch);
int trlda_batch_max_doc_len(const trlda_batch *batch);
/* The number of entries above which a word's list of (document, weight) pairs is walked by a
 * whole workgroup instead of one wavefront in the statistics kernels: 16 << i, the smallest that
 * leaves at most 512 such words in this batch (csrc/estep_kernels.h, kLongWord); and how many
 * words that is. */
int trlda_batch_long_word_len(const trlda_batch *batch);
int trlda_batch_num_long_words(const trlda_batch *batch);
/* Lists of more than 256 .. 1024 entries (a word present in most documents of a large batch; the
 * length is chosen per batch so that there are about a thousand tasks) are cut into segments of at
 * most that many: a segment is a task for a whole workgroup of the statistics kernels, and
 * the workgroup that finishes a word's last segment adds the segments' sums up in segment order
 * (csrc/estep_kernels.h, VeryLongArgs) -- the kernel no longer lasts as long as its longest list
 * (K = 200, 12 500 documents: one list of 12 500 entries kept a workgroup busy for ~100 us).  The
 * number of such words in the batch; trlda_model_set_split_lists(model, 0) keeps every list
 * with one workgroup, for comparisons: same results to rounding. */
int trlda_batch_num_very_long_words(const trlda_batch *batch);

/* ---- device-resident model ---------------------------------------------- */

/* State of TRLDA::LDA (include/lda.h:196-199: mAlpha, mEta, mLambda) kept in HBM.
 * lambda is NOT initialised here: the host mirror draws it with
 * trlda_sample_gamma_init (as src/lda.cpp:71 does) and uploads it. */
int trlda_model_create(trlda_model **out, int device, int K, int V);
int trlda_model_destroy(trlda_model *model);
/* Kernels of this model run on the host's stream from now on (default: a non-blocking stream of
 * the model's own).  The stream must outlive every trlda_batch that was used on it: a batch
 * records the event that guards its memory once, when it is destroyed, on the stream that used
 * it last. */
int trlda_model_set_stream(trlda_model *model, void *hip_stream /* hipStream_t */);
int trlda_model_set_sstats_mode(trlda_model *model, int mode);
/* exp E[log beta] (src/lda.cpp:173) is computed for the words that occur in the batch (the
 * only columns the path reads); dense = 1 fills all V columns like the reference.  The
 * outputs (gamma, sstats) are identical either way. */
int trlda_model_set_dense_preamble(trlda_model *model, int dense);
/* threads per document workgroup in the E-step kernel: 0 = auto, else 64..1024 (x64) */
int trlda_model_set_doc_threads(trlda_model *model, int threads);
/* which document kernels the E-step may use (all give the same results; tests and tuning):
 * AUTO = dual-orientation register kernel for K <= 128 and at most 192 words, else the
 * single-orientation register kernel up to K = 512, else the general (LDS / streaming)
 * kernel; GENERAL = never the single-orientation kernel; WIDE = the single-orientation
 * kernel for every document (K <= 512). */
#define TRLDA_DOCS_AUTO 0
#define TRLDA_DOCS_GENERAL 1
#define TRLDA_DOCS_WIDE 2
/* K <= 32: a WAVE per document of at most 128 words, eight documents per workgroup, no
 * LDS or barrier inside the fixed point (csrc/estep_kernels.h, estep_docs_small_body; round 6); longer
 * documents keep their workgroups -- one each, or a segment each where they are split -- in front of them
 * in the same launch (not where more than half of the documents are longer).  A
 * throughput form -- a document takes 46-55 us on one wave against 30 on eight, but a CU holds eight
 * of them: the default for batches with more short documents than the device has CUs (K = 10, 6400
 * documents: 38.5 against 9.7 M docs/s); _SMALL asks for it at any batch size, _REG for the
 * workgroup-per-document body of K <= 128.  Both leave everything around the body (fused preamble,
 * merged / deferred statistics, lanes) alone. */
#define TRLDA_DOCS_SMALL 3
#define TRLDA_DOCS_REG 4
/* K > 512 always runs the general kernel; it takes K up to TRLDA_VI_MAX_TOPICS (its word rows
 * stay in LDS while they fit, 36 words at K = 513, none from K = 5111; beyond, they are streamed). */
int trlda_model_set_doc_kernel(trlda_model *model, int kind);
/* name (as a profiler lists it, without template arguments) of the document kernel that
 * took most documents of the model's last E-step; "" before the first */
const char *trlda_model_last_doc_kernel(const trlda_model *model);
/* Small tables whose whole batch fits the register-resident document kernel run the row
 * sums and exp(psi(lambda)) in one launch (preamble_fused_kernel) and apply the topic factors
 * exp(-psiSum) in the document kernel; results agree with the two-kernel preamble to a few
 * ulp.  split = 1 always uses the two kernels.  last_preamble_fused: what the last E-step did. */
int trlda_model_set_split_preamble(trlda_model *model, int split);
int trlda_model_last_preamble_fused(const trlda_model *model);
int trlda_model_synchronize(trlda_model *model);
/* K <= 128: a document of 193 .. 1024 words is iterated by ceil(n / 128) workgroups of the
 * document launch, one segment of its words each, which exchange K partial sums per iteration
 * through HBM (src/lda.cpp:189-193 is a sum over the document's words; every segment ends up with
 * bitwise the same gamma) -- a launch lasts as long as its slowest document, and one CU takes
 * ~270 us for 600 words where five take ~50.  enabled = 0: one workgroup per document whatever
 * its length (default 1).  Should a segment ever give up waiting for its peers, the next
 * trlda_model_synchronize / host-copying call fails with TRLDA_ERR_HIP. */
int trlda_model_set_split_docs(trlda_model *model, int enabled);
/* workgroups the model's last document launch used beyond one per document (0: nothing split;
 * a batch whose launch would not end sooner with split documents stays unsplit) */
int trlda_model_last_split_workgroups(const trlda_model *model);
/* Small tables, batches of at most 224 document workgroups (K <= 128 even, a mini-batch of 200):
 * the statistics (src/lda.cpp:207-217) with the M-step (src/onlinelda.cpp:99-100,
 * src/batchlda.cpp:60), the row sums the next E-step needs (src/lda.cpp:172) and its
 * exp(psi(lambda)) can be extra WORKGROUPS OF THE DOCUMENT LAUNCH that wait for a documents-done
 * counter, instead of a kernel of their own behind it: one launch per trust-region iteration
 * (csrc/estep_merged.h).  Same sums in the same order: bitwise the statistics of the stand-alone
 * kernel.  level 1 (default): where the statistics carry an M-step (the update entry points);
 * 2: plain E-steps too (the two forms take the same time there); 0: always the kernel of its
 * own.  last_merged: what the model's last E-step did. */
int trlda_model_set_merged_launch(trlda_model *model, int level);
int trlda_model_set_split_lists(trlda_model *model, int enabled);
int trlda_model_last_merged(const trlda_model *model);

int trlda_model_set_lambda(trlda_model *model, const double *host_lambda /* K x V */);
int trlda_model_get_lambda(trlda_model *model, double *host_lambda /* K x V */);
int trlda_model_set_alpha(trlda_model *model, const double *host_alpha /* K */);
void *trlda_model_lambda_dev(trlda_model *model);   /* K x V fp64, device */
/* sufficient statistics of the last E-step run by trlda_model_online_update /
 * trlda_model_batch_update / trlda_model_estep_host (the model's own workspace): what the
 * adaptive learning rate of src/onlinelda.cpp:167-175 needs (lambdaHat = eta + D/B sstats). */
int trlda_model_get_sstats(trlda_model *model, double *host_sstats /* K x V */);

/*
 * Device-pointer E-step on the model's current lambda: src/lda.cpp:160-220.
 *   gamma_dev  K x B in/out;  sstats_dev K x V out;  iters_dev B int32 or NULL.
 * Launch sequence: row sums -> exp E[log beta] -> per-document
 * fixed point -> per-word sufficient statistics (x exp E[log beta]).
 */
int trlda_model_estep(trlda_model *model, const trlda_batch *batch,
                      double *gamma_dev, double *sstats_dev,
                      int max_iter, double threshold, int32_t *iters_dev);

/* Same, with the initial gamma read from a separate device array (K x B) that is left
 * untouched -- `ArrayXXd gamma = initialGamma` of src/lda.cpp:168 without a device copy. */
int trlda_model_estep_io(trlda_model *model, const trlda_batch *batch,
                         const double *gamma0_dev, double *gamma_dev, double *sstats_dev,
                         int max_iter, double threshold, int32_t *iters_dev);

/* The same, with the batch of the NEXT E-step announced.  Consecutive E-steps on an unchanged
 * lambda are independent of each other, and the document kernel of a 200-document batch leaves
 * 56 of the 256 CUs idle: extra workgroups of this call's document-kernel launch then prepare
 * `next`'s preamble (src/lda.cpp:172-173: row sums, exp(psi(lambda)) on its words) in alternate
 * buffers, and the call that later runs `next` starts with its document kernel.  Nothing is
 * skipped or shared between batches; a wrong or stale announcement (another batch comes, lambda
 * is written in between) just costs the wasted preparation.  Small tables (K <= 128, documents
 * of at most 192 words); elsewhere `next` is ignored.  trlda_model_set_prefetch(model, 0) makes
 * every call prepare its own preamble in a launch of its own. */
int trlda_model_estep_io_next(trlda_model *model, const trlda_batch *batch, const trlda_batch *next,
                              const double *gamma0_dev, double *gamma_dev, double *sstats_dev,
                              int max_iter, double threshold, int32_t *iters_dev);
int trlda_model_set_prefetch(trlda_model *model, int enabled);

/* Deferred statistics for a STREAM of E-steps on an unchanged lambda (a corpus pass of
 * LDA::updateVariablesVI calls, src/lda.cpp:160-220: the statistics of one call, :207-217, feed
 * nothing of the next).  With the switch on, trlda_model_estep_io_next (and through it
 * trlda_model_estep_io_ahead and trlda_model_estep_corpus) returns once its document
 * launch is enqueued; the statistics of that call are formed by extra workgroups of the NEXT
 * trlda_model_estep_io_next call's document launch (on the CUs a 200-document batch leaves idle:
 * a step is then one launch), and are written into the `sstats_dev` THAT call was given.  They
 * are complete -- enqueued on the model's stream ahead of everything that follows -- after the
 * next trlda_model_estep_io_next call or after ANY other call on the model (trlda_model_flush,
 * trlda_model_synchronize, an update, trlda_model_destroy, trlda_batch_destroy of the batch): a
 * caller that reads `sstats_dev` on the stream after one E-step and before the next calls
 * trlda_model_flush first.  gamma and the iteration counts are written by the call itself, as
 * always.  The sums and their order are those of the kernel of its own: bitwise the same
 * statistics.  Same range as the announcement above (small tables, K <= 128 even, batches of at
 * most 256 documents); elsewhere, and for whatever cannot ride along, the statistics are launched
 * as their own kernel.  Only those stream calls defer: every other entry point that runs an E-step
 * (trlda_model_estep, trlda_model_estep_io, trlda_model_estep_host, trlda_model_lower_bound,
 * trlda_model_predictive, the resident and update calls) forms its statistics within the call, with
 * the switch on or off.  Off by default: the Python classes turn it on only inside an EStepStream.
 * trlda_model_last_deferred: bit 0 = the last E-step left its statistics pending, bit 1 = its
 * launch formed the statistics of the call before. */
int trlda_model_set_deferred_stats(trlda_model *model, int enabled);
int trlda_model_flush(trlda_model *model);
int trlda_model_last_deferred(const trlda_model *model);

/* Stream lanes: two E-steps of such a stream in flight at once.  The calls of a corpus pass of
 * LDA::updateVariablesVI (src/lda.cpp:160-220) on an unchanged lambda share nothing but lambda,
 * and a document launch does not end all at once: its documents finish 1-2 us apart (a
 * 129..144-word one 5 us after the others), the helper workgroups at a time of their own.  With
 * two lanes the library deals the stream's calls in turn to two streams of its own (each with the
 * buffers of a model: preamble, factors, pending statistics), so that the next call's workgroups
 * take the CUs as the current one's leave them.
 *   trlda_model_estep_io_ahead   trlda_model_estep_io_next with the batches of the following calls
 *       in order (upcoming[0] is the next call's, upcoming[1] the one after; n_upcoming may be 0):
 *       a lane prepares the preamble of ITS next call, which is two calls ahead.  Identical to
 *       trlda_model_estep_io_next(.., upcoming[0], ..) while lanes are off (the default) or
 *       lambda was last written by an update call (whose kernels leave lambda's row sums behind:
 *       E-steps on that lambda use those).  Any shape goes through the lanes: where deferred
 *       statistics and announcements apply (or are switched on) a call is one launch, elsewhere
 *       its preamble, document and statistics kernels -- whose tails and small launches then run
 *       under the other lane's documents (K = 100, 1600 documents: 188 against 211 us per step).
 *   visibility   gamma, the iteration counts and the statistics of a call that went through a lane
 *       are complete on the model's stream after trlda_model_flush or ANY other call on the model
 *       that is not the next trlda_model_estep_io_ahead -- not after the call itself.  What the
 *       caller enqueued on the model's stream before a call (its gamma0, the last reader of its
 *       output arrays) is waited for by the lane.
 *   outputs   calls in flight together must not share output arrays.  A call whose arrays meet
 *       those of the other lane's outstanding work waits for it (correct, and no faster than one
 *       lane): a streaming caller alternates between two sets of gamma / sstats arrays.
 * Results are those of the one-lane stream, bit for bit.  trlda_model_lane_steps: E-steps that went
 * through the lanes so far. */
int trlda_model_set_stream_lanes(trlda_model *model, int lanes /* 1 or 2 */);
int trlda_model_estep_io_ahead(trlda_model *model, const trlda_batch *batch,
                               const trlda_batch *const *upcoming, int n_upcoming,
                               const double *gamma0_dev, double *gamma_dev, double *sstats_dev,
                               int max_iter, double threshold, int32_t *iters_dev);
/* A corpus pass in ONE call (round 6): LDA::updateVariablesVI (src/lda.cpp:160-220) on an unchanged
 * lambda for every mini-batch of a corpus whose documents lie in HOST memory in CSR form -- `offsets`
 * (n_docs + 1, as trlda_docs_offsets), `ids`, `cnts`; mini-batch i = documents [i * batch_size,
 * min((i + 1) * batch_size, n_docs)) -- the reference's Python loop over do_e_step
 * (python/src/ldainterface.cpp:311-390) with the loop inside the library: batches are made eight ahead
 * of their E-step (trlda_batch_create: index on the worker threads; TRLDA_CORPUS_AHEAD), announced two ahead,
 * stepped through deferred statistics and two lanes (both switched on for the call and put back),
 * destroyed four steps later.  gamma0_dev / gamma_dev: K x n_docs on the device (a document's K
 * values contiguous; gamma0 is only read); the statistics of mini-batch i go to
 * sstats_ring[i % n_ring] (K x V each, n_ring >= 3: whoever wants every batch's statistics passes as
 * many arrays as there are batches); iters_dev: n_docs counts, or NULL.  Everything is complete on
 * the model's stream when the call returns (enqueued: trlda_model_synchronize to wait).  Bitwise the
 * results of the loop of trlda_model_estep_io calls. */
int trlda_model_estep_corpus(trlda_model *model, int64_t n_docs, const int64_t *offsets,
                             const int32_t *ids, const int32_t *cnts, int batch_size,
                             const double *gamma0_dev, double *gamma_dev, double *const *sstats_ring,
                             int n_ring, int max_iter, double threshold, int32_t *iters_dev);
long long trlda_model_lane_steps(const trlda_model *model);
/* What became of the lanes: 0 none made yet (they are made by the first call that goes through them);
 * 2 two lanes on streams that were SEEN to run side by side with each other and with the model's stream
 * -- the runtime hands out hardware queues that are in use once a priority's pool is exhausted, and two
 * lanes on one queue are slower than one lane, so the library makes streams until it holds such a pair
 * (a ~40 us probe kernel on each of two streams: 40 us in all or 80; a marker on one behind a kernel
 * on the other); 1 the lanes were given up -- no such pair was to be had, or the MEASUREMENT said so:
 * after 96 steps through the lanes one launch of a lane and the four that follow it are timed on the
 * device; two launches in flight means a launch LASTS about two steps (51 us where one starts every
 * 26), lanes that do not overlap have launches of one step's length: below 1.0 launches in flight a
 * look says NO (the window ends with the later of the two lanes' launches).  Where a stretch of calls is
 * long enough (64 calls without a flush) every look begins with what the lanes are to beat: eighteen
 * calls in a row on ONE lane, timed the same way -- two lanes that are not 3 % faster than that: NO.  When
 * two of the last four looks said no the lanes are dropped -- the stream of calls goes one launch at a
 * time, as without the switch; a look that said no is followed by the next at once; lanes that pay are
 * kept (on two looks in a row) and looked at AGAIN every 1024 steps for as long as they live: there are
 * process starts in which the launches overlap for a while and then do not.  A window during which the
 * host did not keep the lanes fed is no verdict.  3 two lanes, not looked at (TRLDA_LANE_VERIFY=0).
 * trlda_model_lane_timing: what the last measurement found,
 * microseconds (0: not measured yet). */
int trlda_model_lane_state(const trlda_model *model);
int trlda_model_lane_timing(const trlda_model *model, double *us_per_launch, double *us_per_step);
/* with trlda_model_set_timing on: the summed duration (HIP events on the lanes' streams, one pair per
 * lane around each stretch of calls between joins -- a lane's launches run back to back) and the
 * number of the document launches that went through the lanes; joins the lanes */
int trlda_model_get_lane_timing(trlda_model *model, double *usec_sum, int64_t *launches);

/* Host-pointer convenience around trlda_model_estep (uploads gamma0, downloads
 * gamma / sstats / iters, synchronises). */
int trlda_model_estep_host(trlda_model *model, const trlda_batch *batch,
                           double *gamma, double *sstats,
                           int max_iter, double threshold, int32_t *iters_out);

/* LDA::lowerBound (src/lda.cpp:297-360; python/src/ldainterface.cpp:420-470): an E-step on
 * the batch from gamma (K x B host, in: gamma0, out: gamma), then the variational lower
 * bound with the correction factor = num_documents / B of :302-303 (pass 1 for none).
 * phi is recomputed with the column of the word (the reference's :334 indexes the row; see
 * DESIGN.md "lower bound"). */
int trlda_model_lower_bound(trlda_model *model, const trlda_batch *batch, double *gamma,
                            double eta, double factor, int max_iter, double threshold,
                            double *bound_out);

/* Held-out predictive log-likelihood (Hoffman et al. 2013): VI on `observed` from gamma (K x B
 * host, in: gamma0, out: gamma), then per document d the held-out words' log p(w | d) with
 * E[theta_d] = gamma_d / sum gamma_d and E[beta_kw] = lambda_kw / sum_v lambda_kv.
 * loglik_out[B], tokens_out[B] (host).  Synchronises.
 * loglik_out[d] = sum over the entries (w, c) of `heldout`'s document d of c log p(w | d) (0 for a
 * document without held-out entries; entries with c = 0 add nothing), tokens_out[d] = sum of c.
 * The batches must hold the same number B > 0 of documents, both made for this model's V and
 * device (else TRLDA_ERR_ARG).  csrc/heldout_kernels.h, DESIGN.md 3.12. */
int trlda_model_predictive(trlda_model *model, const trlda_batch *observed,
                           const trlda_batch *heldout, double *gamma, int max_iter,
                           double threshold, double *loglik_out, double *tokens_out);

/* The marginal log-likelihood of whole documents, log p(w_d | alpha, beta), by importance sampling
 * of theta (Wallach, Murray, Salakhutdinov & Mimno 2009, section 4.1; csrc/marginal_kernels.h,
 * DESIGN.md 3.16) with the point estimate beta_kw = lambda_kw / sum_v lambda_kv of
 * trlda_model_predictive.  Per document d with entries (w_i, c_i) and proposal Dir(a_d):
 *   theta^(s) ~ Dir(a_d), s < num_samples
 *   log w_s  = sum_i c_i log(sum_k theta^(s)_k beta_{k, w_i}) + log Dir(theta^(s); alpha) - log Dir(theta^(s); a_d)
 *   loglik_out[d] = logsumexp_s(log w_s) - log num_samples   (nats; exp of it is unbiased for p(w_d))
 *   ess_out[d]    = (sum_s w_s)^2 / sum_s w_s^2, the effective sample size, in [1, num_samples]: far
 *                   below num_samples the estimate rests on a few samples and is poor
 * proposal TRLDA_PROPOSAL_VI: a_d = gamma_d of the E-step of trlda_model_estep_host on the batch
 * (gamma: K x B host, in: gamma0, out: gamma; max_iter, threshold as there); TRLDA_PROPOSAL_PRIOR:
 * a_d = alpha, no E-step runs, the two Dirichlet terms are dropped, gamma is not touched and may be
 * NULL.  A document without entries gets exactly 0 (and ess = num_samples); entries with c = 0 add
 * nothing.  loglik_out[B] host; ess_out[B] host or NULL.
 * The draws are Philox4x32-10 (csrc/philox.h, purposes 19 - 21, counter (s K + k, d, attempt)) under
 * one key of trlda_rng_draw_key, drawn by every call that passes the argument checks (also for an
 * empty batch): a document's value is a function of the key, its index d in the batch, its entries
 * and the model -- not of the batch around it.  TRLDA_ERR_ARG, before anything is drawn, copied or
 * launched: K above TRLDA_VI_MAX_TOPICS (either proposal), an unknown proposal, num_samples < 1,
 * num_samples * K >= 2^32, a batch of another V or device.  lambda, alpha and the counters are left
 * alone; with TRLDA_PROPOSAL_VI trlda_model_get_sstats holds that E-step's statistics afterwards.
 * Synchronises.  No reference counterpart. */
#define TRLDA_PROPOSAL_VI    0
#define TRLDA_PROPOSAL_PRIOR 1
int trlda_model_document_loglik(trlda_model *model, const trlda_batch *batch, double *gamma,
                                int proposal, int num_samples, int max_iter, double threshold,
                                double *loglik_out, double *ess_out);

/* The marginal log-likelihood of whole documents, log p(w_d | alpha, beta), by the left-to-right
 * sequential sampler (Wallach, Murray, Salakhutdinov & Mimno 2009, Algorithm 3; Buntine 2009;
 * csrc/l2r_kernels.h) with the point estimate beta of trlda_model_predictive.  It
 * samples the tokens' topics, not theta, and has no proposal.  Per document d with tokens w_0 ..
 * w_{N-1} (the entries in order, an entry giving c > 0 consecutive tokens), particle r <
 * num_particles and position n, with n_k the counts of the prefix's current topics:
 *   resample != 0: for t = 0 .. n-1: take z_t out, z_t ~ beta_{k, w_t} (alpha_k + n_k), put it back
 *   z_n ~ beta_{k, w_n} (alpha_k + n_k); p_r(n) = (sum_k beta_{k, w_n} (alpha_k + n_k)) / (sum alpha + n)
 * resample = 0 is the O(N) sequential sampler, otherwise the work is O(N^2) per particle.
 *   TRLDA_L2R_PARTICLE  loglik_out[d] = logsumexp_r(sum_n log p_r(n)) - log num_particles: exp of it
 *                       is unbiased for p(w_d) for any number of particles
 *   TRLDA_L2R_POSITION  loglik_out[d] = sum_n log(mean_r p_r(n)), Algorithm 3 as published: biased
 *                       for num_particles > 1 (DESIGN.md 3.17 has the figures); with one particle
 *                       the two are the same bits
 * A document without tokens gets exactly 0.  loglik_out[B] host; tokens_out[B] host or NULL: N_d.
 * The draws are Philox4x32-10 (csrc/philox.h, purposes 22 / 23, counter (token, position,
 * d * num_particles + r)) under one key of trlda_rng_draw_key, drawn by every call that passes its
 * checks (also for an empty batch): a document's value is a function of the key, its index d, its
 * entries, num_particles and the model -- not of the batch around it nor of how the batch is cut
 * into groups against the workspace.  TRLDA_ERR_ARG, before anything is drawn or launched:
 * num_particles < 1, B * num_particles >= 2^32, an unknown combine, K > 1024 (the Gibbs path's
 * limit), a batch of another V or device; and, before the key is drawn, a single document with
 * N_d * num_particles above the workspace (2^23 token-particles; the environment's TRLDA_L2R_BUDGET
 * replaces the figure, for tests).  TRLDA_ERR_VALUE with the Gibbs path's message when a histogram
 * does not sum to a positive finite number.  lambda, alpha and the counters are left alone.
 * Synchronises.  No reference counterpart. */
#define TRLDA_L2R_PARTICLE 0
#define TRLDA_L2R_POSITION 1
int trlda_model_left_to_right(trlda_model *model, const trlda_batch *batch, int num_particles,
                              int resample, int combine, double *loglik_out, double *tokens_out);

/* The per-word topic posteriors of the variational path: the phi that LDA::updateVariablesVI forms
 * inside its fixed point and drops (src/lda.cpp:189-197; csrc/wordtopics_kernels.h).
 * An E-step on the batch from gamma (K x B host, in: gamma0, out: gamma; max_iter, threshold as for
 * trlda_model_estep_host), then per entry p = (d, w_p, c_p) of the batch's CSR, in the batch's own
 * entry order,
 *   s_pk = exp(psi(gamma_dk) - psi(rs_k)) exp(psi(lambda_{k, w_p})),  rs_k = sum_v lambda_kv
 *   phi_pk = s_pk / sum_j s_pj
 * topics_out[p * top_n + r] (int32) and probs_out[p * top_n + r] (fp64), r < top_n: the top_n topics
 * of row p in decreasing phi, equal values by smaller topic id first (the rule of
 * trlda_model_top_words); host arrays of trlda_batch_nnz(batch) * top_n elements.  With top_n = K a
 * row of probs_out is the whole posterior in ranked order.  An entry with c_p = 0 gets a row like
 * any other (the row depends on w_p and gamma_d only); a document without entries has no rows; an
 * empty batch writes nothing.  The order of the additions in a row's sum depends on K alone: a
 * document's rows are bitwise the same alone and inside any batch for the same gamma column.
 * TRLDA_ERR_ARG, before anything is waited for, copied or launched: K above TRLDA_VI_MAX_TOPICS,
 * top_n outside [1, min(K, 32)], a batch of another V or device.  lambda, alpha and the counters are
 * left alone; pending deferred statistics and stream lanes are settled first; afterwards
 * trlda_model_get_sstats holds that E-step's statistics, as after trlda_model_document_loglik with
 * TRLDA_PROPOSAL_VI.  Synchronises.  No reference counterpart. */
int trlda_model_word_topics(trlda_model *model, const trlda_batch *batch, double *gamma, int top_n,
                            int max_iter, double threshold, int32_t *topics_out, double *probs_out);

/* The same rows from a gamma the caller keeps on the device (K x B, read only: no E-step runs, the
 * model's statistics keep what they held), into device arrays of trlda_batch_nnz(batch) * top_n
 * elements.  Enqueued on the model's stream; does not synchronise.  The same checks; on the same
 * gamma bitwise the rows of trlda_model_word_topics. */
int trlda_model_word_topics_dev(trlda_model *model, const trlda_batch *batch, const double *gamma_dev,
                                int top_n, int32_t *topics_dev, double *probs_dev);

/* Topic coherence (Mimno et al. 2011; Bouma 2009): the top words of each topic and the document
 * counts of word lists, on the device (csrc/coherence_kernels.h).  The per-pair
 * formulas are the caller's (host) arithmetic on the counts.  No reference counterpart. */

/* words_out (K x top_n int32, host, topic-major: [k * top_n + r]) = the top_n word ids of each
 * topic in decreasing order of lambda_kw, equal values by smaller id first -- the order of
 * np.lexsort((arange(V), -lambda[k])); NaN after every number.  1 <= top_n <= min(V, 100), else
 * TRLDA_ERR_ARG.  Pending deferred statistics and stream lanes are settled first.  Synchronises. */
int trlda_model_top_words(trlda_model *model, int top_n, int32_t *words_out);

/* A counting accumulator for T word lists of N ids each (words: T x N int32, host, row-major;
 * 1 <= T, 2 <= N <= 100, ids in [0, V) and distinct within a row, else TRLDA_ERR_ARG), made for
 * `model`'s V and device; it runs on the model's stream and must be destroyed before the model.
 * Its counts stay on the device between batches. */
typedef struct trlda_cooc trlda_cooc;
int trlda_cooc_create(trlda_model *model, const int32_t *words, int T, int N, trlda_cooc **out);
/* Adds a batch (made for the model's V and device, else TRLDA_ERR_ARG): document d contains word w
 * when it has an entry (w, c) with c > 0.  Asynchronous; the batch may be destroyed at once. */
int trlda_cooc_add(trlda_cooc *cooc, const trlda_batch *batch);
/* The counts so far (host): doc_freq[T x N] (documents that contain word (t, i)),
 * co_doc_freq[T x N x N] (documents that contain words (t, i) and (t, j); symmetric, doc_freq on
 * the diagonal), *num_docs (documents added, empty ones included).  Synchronises. */
int trlda_cooc_read(trlda_cooc *cooc, int64_t *doc_freq, int64_t *co_doc_freq, int64_t *num_docs);
int trlda_cooc_destroy(trlda_cooc *cooc);

/* Spectral initialisation (csrc/anchor_kernels.h): the word co-occurrence matrix Q of
 * a corpus stream, FastAnchorWords on its row-normalised form and RecoverL2 (Arora et al. 2013).  The
 * accumulator is made for `model`'s V and device, runs on the model's stream and must be destroyed
 * before the model.  Q (V rows of stride ceil(V / 4) * 4 doubles) and, from the first selection or
 * recovery on, one work copy of the same size live on the device: when the two exceed max_bytes the
 * call fails with TRLDA_ERR_ARG and a message naming the bytes needed, before anything is allocated.
 * No reference counterpart. */
typedef struct trlda_anchor trlda_anchor;
int trlda_anchor_create(trlda_model *model, size_t max_bytes, trlda_anchor **out);
/* Adds a batch (made for the model's V and device, else TRLDA_ERR_ARG).  A document with counts c and
 * n = sum c >= 2 adds ((int64) c_w c_v - [w = v] c_w) / (double)(n (n - 1)) -- an exact integer, one
 * division -- to Q_wv for every pair of its entries; the others are skipped and counted.  Row w belongs
 * to one workgroup that walks w's documents in ascending order: one addition per (document, pair), in
 * document order across the stream, no floating-point atomics -- Q is symmetric bit for bit and does
 * not depend on how the corpus is cut into batches.  A batch with a negative count, or one that lists a
 * word twice in a document, fails with TRLDA_ERR_VALUE and adds nothing.  The call waits once, for the
 * repeated-word flag of the batch's entries; the row kernel is still running when it returns -- on the
 * model's stream, which every reader of Q follows, and the batch may be destroyed at once. */
int trlda_anchor_add(trlda_anchor *acc, const trlda_batch *batch);
/* Replaces Q by the V x V row-major host matrix (finite, non-negative and symmetric bit for bit, else
 * TRLDA_ERR_VALUE) and doc_freq by the V given values (NULL: none -- no threshold applies to the
 * candidates then); the other counters are cleared. */
int trlda_anchor_load(trlda_anchor *acc, const double *Q, const int64_t *doc_freq);
/* doc_freq[V] (contributing documents with an entry (w, c), c > 0), word_count[V] (their counts of w)
 * and counters[3]: documents that contributed, documents skipped, tokens of the contributing ones. */
int trlda_anchor_counts(trlda_anchor *acc, int64_t *doc_freq, int64_t *word_count, int64_t *counters);
/* Rows of Q into out (n x V, host): rows[i] (in [0, V)), or the first n rows when rows is NULL. */
int trlda_anchor_read(trlda_anchor *acc, const int32_t *rows, int n, double *out);
/* r[V], the row sums of Q, and *total, the sum of r.  The order of every sum of n values here: thread
 * t of 256 adds the values t, t + 256, ... in ascending order from +0, then the 256 partial sums are
 * folded as p[t] += p[t + s] for s = 128, 64, ..., 1. */
int trlda_anchor_row_sums(trlda_anchor *acc, double *r, double *total);
/* FastAnchorWords: `num` anchors among the candidates -- words with r_w > 0 and, when min_doc_freq >= 0,
 * doc_freq >= min_doc_freq; fewer candidates than anchors is TRLDA_ERR_VALUE.  The work copy holds the
 * rows Q_w / r_w.  Round 0 takes the candidate row of the largest squared norm and subtracts it from
 * every candidate row; each later round takes the largest squared residual norm, divides that row by
 * its norm and takes its component out of every candidate row (modified Gram-Schmidt on the work
 * copy; norms and dot products in the order above; the winner in the order norm^2 descending, word id
 * ascending; a chosen word leaves the candidates).  ids[num] in selection order, score[num] the
 * winning norm^2 of each round, runner[num] the runner-up's (-1 when there is none). */
int trlda_anchor_select(trlda_anchor *acc, int num, int64_t min_doc_freq, int32_t *ids, double *score,
                        double *runner);
/* RecoverL2 for the A anchors (distinct, in [0, V), A <= 640, else TRLDA_ERR_ARG): H = Qbar Qbar_S'
 * (V x A) by the staged fp64 tile product over the words in ascending chunks, G = its anchors' rows, and
 * per word, a wave each, min over the simplex of |Qbar_w - x' Qbar_S|^2 by projected gradient with
 * Nesterov's momentum and gradient restart, step 1 / (2 max_i sum_j |G_ij|), from x = 1 / A, the exact
 * projection (Michelot), until the word's Frank-Wolfe gap is at most tol |Qbar_w|^2 or max_iter
 * iterations have run.  beta[V x A] (word-major: K x V in Fortran order): x_wk p_w normalised over w,
 * p_w = r_w / total; pi[A]: the columns' masses; unless NULL, x[V x A], iters[V] and gaps[V] (the final
 * gap / |Qbar_w|^2).  A word's result depends on its row, the anchors' rows and A alone. */
int trlda_anchor_recover(trlda_anchor *acc, const int32_t *anchors, int A, double tol, int max_iter,
                         double *beta, double *pi, double *x, int32_t *iters, double *gaps);
/* 0 (default): the solver holds G in LDS up to 128 anchors and reads it from global memory above;
 * 1: always from global memory.  The results are the same bit for bit. */
int trlda_anchor_set_gram_lds(trlda_anchor *acc, int mode);
int trlda_anchor_destroy(trlda_anchor *acc);

/* Nearest documents in topic space (csrc/docindex_kernels.h): a table of the
 * documents' topic proportions theta = gamma / sum(gamma) on the model's device, and the top_n
 * nearest indexed documents of each document of a batch.  measure TRLDA_MEASURE_HELLINGER stores
 * r_k = sqrt(theta_k), TRLDA_MEASURE_COSINE r_k = theta_k / sqrt(sum_j theta_j^2); the similarity is
 * s(q, d) = sum_k r_qk r_dk (the Bhattacharyya coefficient / the cosine).  A row depends on its gamma
 * column and K alone, s on the two rows and K alone; the ranking is the total order (s descending,
 * id ascending), ids being the positions in order of addition from 0.  The index runs on the
 * model's stream and must be destroyed before the model; it stores theta, not lambda: rows added
 * before lambda changed are stale, which is not detected.  No reference counterpart. */
#define TRLDA_MEASURE_HELLINGER 0
#define TRLDA_MEASURE_COSINE    1
typedef struct trlda_docindex trlda_docindex;
/* An empty index for `model`'s K and device (an unknown measure: TRLDA_ERR_ARG).  No reference
 * counterpart. */
int trlda_docindex_create(trlda_model *model, int measure, trlda_docindex **out);
/* Room for `rows` documents in all.  Without it the table doubles from max(1024, first batch) with a
 * device-to-device copy on the model's stream each time.  No reference counterpart. */
int trlda_docindex_reserve(trlda_docindex *index, int64_t rows);
/* An E-step on the batch as trlda_model_estep_host runs it (gamma: K x B host, in: gamma0, out:
 * gamma; afterwards trlda_model_get_sstats holds that E-step's statistics, as after
 * trlda_model_word_topics), then the B rows are appended.  TRLDA_ERR_ARG, before anything is waited
 * for, copied or launched: K above TRLDA_VI_MAX_TOPICS, a batch of another V or device.  lambda,
 * alpha and the counters are left alone; pending deferred statistics and stream lanes are settled
 * first.  Synchronises.  No reference counterpart. */
int trlda_docindex_add(trlda_docindex *index, const trlda_batch *batch, double *gamma, int max_iter,
                       double threshold);
/* Appends the rows of B gamma columns (K x B host; any K >= 1; every value finite and positive,
 * else TRLDA_ERR_VALUE and nothing is added).  No E-step, nothing drawn.  Synchronises.  No reference
 * counterpart. */
int trlda_docindex_add_gamma(trlda_docindex *index, const double *gamma_host, int B);
/* The same from a gamma on the device (not validated).  Enqueued on the model's stream; does not
 * synchronise.  On the same gamma bitwise the rows of trlda_docindex_add_gamma.  No reference
 * counterpart. */
int trlda_docindex_add_gamma_dev(trlda_docindex *index, const double *gamma_dev, int B);
/* Documents indexed so far: the next id.  No reference counterpart. */
int64_t trlda_docindex_size(const trlda_docindex *index);
/* An E-step on the batch as in trlda_docindex_add, then per document the top_n nearest indexed
 * documents: ids_out (int64) and sim_out (fp64, the similarity s), host, B x top_n row-major, best
 * first.  TRLDA_ERR_ARG, before anything is waited for, copied or launched: an empty index, top_n
 * outside [1, min(size, 100)], K above TRLDA_VI_MAX_TOPICS, a batch of another V or device.  The
 * index is left as it was.  Synchronises.  No reference counterpart. */
int trlda_docindex_query(trlda_docindex *index, const trlda_batch *batch, double *gamma, int max_iter,
                         double threshold, int top_n, int64_t *ids_out, double *sim_out);
/* The same search for B gamma columns given on the host (K x B; any K >= 1; finite and positive,
 * else TRLDA_ERR_VALUE): no E-step, nothing drawn.  On the same gamma bitwise the results of
 * trlda_docindex_query.  Synchronises.  No reference counterpart. */
int trlda_docindex_query_gamma(trlda_docindex *index, const double *gamma_host, int B, int top_n,
                               int64_t *ids_out, double *sim_out);
/* Rows first .. first + count - 1 as stored (count x K host, row-major, without the zero pad);
 * rows outside [0, size): TRLDA_ERR_ARG.  Synchronises.  No reference counterpart. */
int trlda_docindex_read_rows(trlda_docindex *index, int64_t first, int64_t count, double *rows_out);
/* A/B switch for tests and measurements: index rows per workgroup of the search (a positive multiple
 * of 16; 0: the default, 2048).  The results do not depend on it.  No reference counterpart. */
int trlda_docindex_set_slab_rows(trlda_docindex *index, int rows);
int trlda_docindex_destroy(trlda_docindex *index);

/* Topic summaries of an indexed corpus (csrc/topicdocs_kernels.h).  theta^ is theta
 * recovered from the stored row r: r_k * r_k (hellinger, one IEEE multiply) or r_k / sum_j r_j (cosine,
 * IEEE division, the sum in the order the rows' kernel adds sum gamma); it depends on the row and K
 * alone.  Every call below runs on the model's stream, synchronises, keeps its temporaries to itself
 * and leaves the index, lambda, alpha, the model's statistics and the generator as they were; nothing
 * is atomic: two calls agree bitwise, however the index was filled.  TRLDA_ERR_ARG, before anything is
 * waited for, copied or launched: a NULL index or required output, an empty index, top_n outside
 * [1, min(size, 100)].
 *
 * Per topic k the first top_n documents in the total order (theta^_dk descending, id ascending):
 * ids_out (int64) and, unless NULL, theta_out (fp64, their theta^_dk), host, topic-major
 * [k * top_n + r].  The result does not depend on trlda_docindex_set_slab_rows.  No reference
 * counterpart. */
int trlda_docindex_topic_documents(trlda_docindex *index, int top_n, int64_t *ids_out,
                                   double *theta_out /* may be NULL */);
/* The mean m_k = (sum_d theta^_dk) / N (mean_out, K) and the centred scatter
 * S_ij = sum_d (theta^_di - m_i)(theta^_dj - m_j) (scatter_out, K x K, bitwise symmetric) of the N
 * indexed documents, in two passes: centring before the product avoids the cancellation of
 * sum theta theta^T / N - m m^T.  The covariance is S / (N - ddof).  No reference counterpart. */
int trlda_docindex_topic_moments(trlda_docindex *index, double *mean_out /* K */,
                                 double *scatter_out /* K x K */);
/* A/B switch for tests and measurements: index rows per chunk of the scatter's sum over N (0: the
 * default, a function of (K, N) alone).  Results with a forced chunk agree within rounding, not
 * bitwise.  No reference counterpart. */
int trlda_docindex_set_moment_chunk(trlda_docindex *index, int rows);

/* Indexed documents by query likelihood (csrc/querylik_kernels.h; the LDA term of Wei &
 * Croft's LBDM, SIGIR 2006).  Nothing is inferred for a query: document d scores
 *   score(q, d) = sum_i c_i log P(d, w_i),  P(d, w) = sum_k theta^_dk lambda_kw / R_k,  R_k = sum_v lambda_kv
 * over the batch's entries (w_i, c_i) of query q, in nats, with theta^ as above, the model's lambda at the
 * time of the call and the row sums formed from it as trlda_model_recommend forms them.  An entry with
 * c_i <= 0 adds nothing; a query without entries scores 0.0 everywhere; P = 0 gives -inf (ranked last, by
 * id); no NaN arises.  Per query the first top_n documents in the total order (score descending, id
 * ascending): ids_out (int64) and loglik_out (fp64), host, B x top_n row-major.  Every P is one chain of
 * v_mfma_f64_16x16x4_f64 over ascending k and the terms of a score are added in an order that depends
 * on the entry's position within its query alone; nothing is atomic: a query's result is bitwise the
 * same alone and inside any batch, whatever trlda_docindex_set_slab_rows says and however the index was
 * filled, and a document's score does not depend on the other rows of the index.  TRLDA_ERR_ARG, before
 * anything is waited for, copied or launched: a NULL index, an empty index, top_n outside
 * [1, min(size, 100)], a batch of another V or device; and, after the row-sum pass and before any other
 * kernel, a row sum of lambda that is not finite and positive.  Any K >= 1: no E-step runs.  Nothing is
 * drawn; the index, lambda, alpha, the counters and the model's statistics are left alone; pending
 * deferred statistics and stream lanes are settled first; the temporaries are the call's own.  The index
 * stores theta, not lambda: rows added before lambda changed are stale, which is not detected.
 * Synchronises.  No reference counterpart. */
int trlda_docindex_query_likelihood(trlda_docindex *index, const trlda_batch *batch, int top_n,
                                    int64_t *ids_out, double *loglik_out);

/* The document groups of an indexed corpus (csrc/cluster_kernels.h): spherical k-means
 * on the stored rows, which is Lloyd's algorithm for the index's own measure -- both measures store
 * unit-length rows x, so the squared Hellinger distance, like the cosine distance, is 1 - <x, m>.
 * Centroids are given and returned as K x C positive, finite topic proportions laid out like a gamma;
 * a column's row is the row trlda_docindex_add_gamma would store for it, bitwise.
 *   s(n, c) = sum_k x_nk m_ck   one chain of v_mfma_f64_16x16x4_f64 over ascending k: the two rows and
 *                               K alone decide it
 *   label(n)                    the first c in the total order (s descending, c ascending);
 *                               sim(n) = s(n, label(n))
 *   m_c = S_c / |S_c|           S_c = the sum of the rows labelled c, ids ascending, in chunks of 256
 *                               members added in chunk order; |S_c|^2 in the order the rows' kernel adds
 *                               its sums: the member set and K alone decide it.  A cluster without
 *                               members keeps its row.
 * Nothing is atomic in floating point: two calls agree bitwise, whatever trlda_docindex_set_slab_rows
 * says and however the index was filled.  TRLDA_CLUSTER_MAX_CLUSTERS (4096) bounds C.  TRLDA_ERR_ARG,
 * before anything is waited for, copied or launched: a NULL index or required output, an empty index,
 * C outside [1, min(size, 4096)], max_iter < 0, B < 1 with a gamma; TRLDA_ERR_VALUE, with nothing
 * changed: a centroid or gamma value that is not finite and positive.  Any K >= 1: no E-step runs.
 * Nothing is drawn; the index, lambda, alpha, the counters and the model's statistics are left alone;
 * pending deferred statistics and stream lanes are settled first; the temporaries are the call's own.
 * Both calls synchronise.
 *
 * One assignment.  With gamma_host NULL the N indexed documents are labelled (B is ignored), otherwise
 * the B columns of gamma_host (K x B), whose rows are formed as trlda_docindex_query_gamma forms them:
 * labels_out (int32) and, unless NULL, sim_out (fp64), one per document.  No reference counterpart. */
int trlda_docindex_assign(trlda_docindex *index, const double *centroids_host /* K x C */, int C,
                          const double *gamma_host /* K x B or NULL */, int B, int32_t *labels_out,
                          double *sim_out /* may be NULL */);
/* The loop: assign; if this is not the first assignment and no label changed, stop (*converged_out = 1);
 * otherwise, if fewer than max_iter updates have run, update the centroids and assign again.  The last
 * step is an assignment, so labels_out (int32, N) and sim_out (fp64, N) are the assignment under the
 * returned centroids; *iterations_out is the number of updates that ran; max_iter = 0 is one
 * assignment.  The count of changed labels is an integer formed on the device, read once per
 * iteration.  sizes_out (int64, C): the members of each cluster under labels_out.  centroids (K x C
 * host; in: the initial ones, out: the final ones) returns theta^ of the final rows, recovered as
 * trlda_docindex_topic_documents recovers it.  No reference counterpart. */
int trlda_docindex_cluster(trlda_docindex *index, int C, double *centroids /* K x C */, int max_iter,
                           int32_t *labels_out, double *sim_out /* may be NULL */,
                           int64_t *sizes_out /* may be NULL */, int *iterations_out, int *converged_out);

/* The exact silhouette (Rousseeuw 1987) of indexed documents under a labelling, in the index's own
 * distance (csrc/silhouette_kernels.h).  labels_host (int32, N = the index's size) holds
 * values in [0, C); a value without members is allowed and ignored.  With ids_host NULL the N documents
 * are scored (M is ignored), otherwise the M rows ids_host names, in any order and with repeats, each
 * against ALL N documents.
 *   d(i, j)       sqrt(max(0, 1 - s_ij)) (hellinger) or max(0, 1 - s_ij) (cosine); s_ij the dot of the two
 *                 stored rows, one chain of v_mfma_f64_16x16x4_f64 over ascending k as in
 *                 trlda_docindex_assign.  The pair (i, i) is left out by id, not by value.
 *   a(i)          sum_{j in own, j != i} d(i, j) / (n_own - 1)
 *   b(i)          the smallest sum_{j in c} d(i, j) / n_c over the non-empty c != own; neighbour(i) the
 *                 first such c in the total order (mean ascending, c ascending)
 *   sil(i)        (b - a) / max(a, b); 0 where n_own = 1 (a = 0; b and neighbour are still reported) and
 *                 where max(a, b) = 0
 * A cluster's members are added by ascending id: the member of rank r joins partial sum r mod 16, the 16
 * partial sums are added in a fixed tree, so sum_{j in c} d(i, j) depends on row i, the member set of c
 * and K alone -- not on the other clusters, on c's number, on trlda_docindex_set_slab_rows, on which
 * other rows are scored or on how the index was filled; two calls agree bitwise.  Nothing of size
 * M x N or M x C exists.  sil_out, a_out, b_out (fp64) and neighbour_out (int32) hold one value per
 * scored row.  TRLDA_ERR_ARG, before anything is waited for, copied or launched: a NULL index, labels
 * or sil_out, an empty index, C outside [2, 4096], M < 1 with ids; TRLDA_ERR_VALUE, with nothing changed
 * (counted on the host): a label outside [0, C), an id outside [0, N), fewer than two clusters with
 * members.  Nothing is drawn; the index, lambda, alpha, the counters and the model's statistics are left
 * alone; pending deferred statistics and stream lanes are settled first; the temporaries are the call's
 * own.  Synchronises.  No reference counterpart. */
int trlda_docindex_silhouette(trlda_docindex *index, const int32_t *labels_host /* N */, int C,
                              const int64_t *ids_host /* M or NULL: all N */, int64_t M, double *sil_out,
                              double *a_out /* may be NULL */, double *b_out /* may be NULL */,
                              int32_t *neighbour_out /* may be NULL */);

/* The radius join of an indexed corpus (csrc/neighbors_kernels.h): for each scored row
 * the indexed documents within distance `radius` of it, as a CSR list.  The M scored rows are the stored
 * rows ids_host names (any order, repeats allowed; NULL with gamma_host NULL too: all N, row q is
 * document q and M is ignored), or the rows of the M columns of gamma_host (K x M), formed as
 * trlda_docindex_query_gamma forms them; not both.
 *   s(i, j)       the dot of scored row i and stored row j, one chain of v_mfma_f64_16x16x4_f64 over
 *                 ascending k as in trlda_docindex_silhouette: it depends on the two rows and K alone, and
 *                 s(i, j) and s(j, i) are the same bits
 *   d(i, j)       sqrt(fmax(1 - s, 0)) (hellinger) or fmax(1 - s, 0) (cosine), formed on the device
 *   hit           d <= radius.  Where the scored rows are stored rows the pair (i, i) is left out by id, not
 *                 by value; for gamma rows nothing is left out.
 * Three steps on the device: the hits are counted per (scored row, slab of columns); an exclusive prefix
 * over the counts in (row, slab) order gives every slab's place and indptr_out (int64, M + 1;
 * indptr_out[M] is the total); the same products and the same predicate, from the same device function,
 * then put every hit at a place that depends on the data alone.  Row q's hits are ids_out[indptr_out[q]
 * ... indptr_out[q + 1] - 1] (int64) in ascending id, val_out (fp64, may be NULL) their d, or their s
 * with want_similarity != 0.  The result does not depend on trlda_docindex_set_slab_rows (rounded up to
 * a multiple of 64 columns here; 0: a default sized so that few scored rows still fill the device), on
 * the rows scored beside a row or on how the index was filled; two calls agree bitwise.  No atomics;
 * nothing of size M x N exists.  Any K >= 1: no E-step runs.
 * The count and the prefix always run.  With ids_out NULL the call ends there (one product formed).  If
 * indptr_out[M] > capacity nothing is written to ids_out / val_out and the call still returns TRLDA_OK:
 * the caller compares the two and calls again.  Otherwise the first indptr_out[M] entries are written.
 * TRLDA_ERR_ARG, before anything is waited for, copied or launched: a NULL index or indptr_out, an empty
 * index, both ids_host and gamma_host, M < 1 with either, capacity < 0, val_out without ids_out;
 * TRLDA_ERR_VALUE, with nothing changed: a radius that is not finite or is negative, an id outside
 * [0, N), a gamma value that is not finite and positive.  Nothing is drawn; the index, lambda, alpha, the
 * counters and the model's statistics are left alone; pending deferred statistics and stream lanes are
 * settled first; the temporaries are the call's own.  Synchronises.  No reference counterpart. */
int trlda_docindex_neighbors(trlda_docindex *index, double radius, const int64_t *ids_host /* M or NULL */,
                             const double *gamma_host /* K x M or NULL */, int64_t M, int want_similarity,
                             int64_t capacity, int64_t *indptr_out /* M + 1 */,
                             int64_t *ids_out /* capacity, or NULL: count only */,
                             double *val_out /* capacity, or NULL */);

/* One round's sweep of Boruvka's algorithm on the complete graph over the N indexed documents
 * (csrc/mst_kernels.h): per document its lightest edge to a document of another component.
 *   s(i, j), d(i, j)  as in trlda_docindex_neighbors, bit for bit
 *   w(i, j)           fmax(d, fmax(core_host[i], core_host[j])), the mutual-reachability distance of
 *                     HDBSCAN*; d itself with core_host NULL.  w(i, j) and w(j, i) are the same bits.
 *   candidate         j of i iff comp_host[j] != comp_host[i] and j != i
 *   best_out[i]       the first candidate of i in the order (w ascending, j ascending) -- for a fixed i the
 *                     edge order (w, min(i, j), max(i, j)), a strict total order on the edges, so that
 *                     joining every component along its lightest outgoing edge closes no cycle -- and
 *                     weight_out[i] its w; -1 and +inf for a document without a candidate.
 * The two arrays are uploaded, one kernel runs on the model's stream, the results are downloaded and the
 * call waits once.  A workgroup takes trlda_docindex_set_slab_rows rows of the table (0: whole passes of
 * 128 rows, sized so that the grid stays near 1024 workgroups); the result does not depend on it or on how
 * the index was filled; two calls agree bitwise.  No atomics; nothing of size N x N exists.  Any K >= 1: no E-step runs.
 * TRLDA_ERR_ARG, before anything is waited for, copied or launched: a NULL index, comp_host, best_out or
 * weight_out, an empty index, more than INT_MAX documents; TRLDA_ERR_VALUE, with nothing changed: a core
 * distance that is not finite or is negative.  Nothing is drawn; the index, lambda, alpha, the counters and
 * the model's statistics are left alone; pending deferred statistics and stream lanes are settled first;
 * the temporaries are the call's own.  No reference counterpart. */
int trlda_docindex_mst_sweep(trlda_docindex *index, const int32_t *comp_host /* N */,
                             const double *core_host /* N or NULL */, int64_t *best_out /* N */,
                             double *weight_out /* N */);

/* A 2-D map of an indexed corpus: exact t-SNE (van der Maaten & Hinton 2008) on the stored rows
 * (csrc/tsne_kernels.h).  No reference counterpart.  Every call below checks its
 * arguments before anything is waited for, copied or launched (TRLDA_ERR_ARG; TRLDA_ERR_VALUE for
 * values, counted on the host, with nothing changed), draws nothing, leaves the index, lambda, alpha, the
 * counters and the model's statistics alone, settles pending deferred statistics and stream lanes first,
 * runs on the model's stream, synchronises once at its end and keeps no device buffer of its own beyond
 * the index's grow-only query workspaces.  No floating-point atomics; two calls agree bitwise.
 *
 * trlda_docindex_nearest: per indexed document its top_n nearest OTHER documents, 1 <= top_n <=
 * min(N - 1, 99), in the total order of trlda_docindex_query (s descending, id ascending) with the
 * document's own id removed: top_n + 1 entries are ranked with the table's own rows as the query rows
 * (no gamma, no copy of the table), the entry with the own id is dropped, or the last one where the own
 * id is not among them (more than top_n exact duplicates of smaller id).  ids_out (int64) and sim_out
 * (fp64, the similarity s) are N x top_n row-major.  The rows are scored block_rows at a time (0:
 * automatic); the result does not depend on it, on trlda_docindex_set_slab_rows or on how the index was
 * filled. */
int trlda_docindex_nearest(trlda_docindex *index, int top_n, int block_rows, int64_t *ids_out /* N x top_n */,
                           double *sim_out /* N x top_n */);
/* The conditional affinities of the k = min(N - 1, floor(3 perplexity)) nearest neighbours, 1 <=
 * perplexity <= 33, from the device-resident form of trlda_docindex_nearest.  With D_j = fmax(1 - s_j, 0)
 * (the squared Hellinger distance, or the cosine distance), d_j = D_j - D_first, w_j = exp(-beta d_j),
 * S = sum w_j: p_j = w_j / S with beta such that H(beta) = log S + beta sum w_j d_j / S = log perplexity,
 * found by doubling from 1 / mean(d) and bisection to hi - lo <= hi 2^-50 (at most 200 steps; beta = hi).
 * Two limits: log k <= log perplexity gives beta = 0 and p = 1 / k; m >= perplexity exactly tied
 * nearest (d_j = 0) gives beta = +inf and p = 1 / m on those m, 0 elsewhere.  ids_out (int64) and p_out
 * (fp64) are N x k row-major in the order of trlda_docindex_nearest, beta_out (fp64) holds N values. */
int trlda_docindex_affinities(trlda_docindex *index, double perplexity, int block_rows, int64_t *ids_out,
                              double *p_out, double *beta_out);
/* A/B switch: rows per workgroup of the repulsion kernel, 0 (default, 256) or a multiple of 64 up to 1024.
 * Results do not depend on it. */
int trlda_docindex_set_tsne_tile(trlda_docindex *index, int rows);
/* y_out (N x 2 row-major) = (theta^ - mean) axes: theta^ recovered from the stored rows as
 * trlda_docindex_topic_documents recovers it, mean_host K values, axes_host 2 x K (axis c at
 * axes_host[c K ...]).  The PCA start of a map: the caller passes the two leading eigenvectors of the
 * scatter of trlda_docindex_topic_moments, scaled as it likes. */
int trlda_docindex_tsne_project(trlda_docindex *index, const double *mean_host /* K */,
                                const double *axes_host /* 2 x K */, double *y_out /* N x 2 */);
/* The t-SNE gradient and KL divergence of the map y (N x 2 row-major, host, finite) under the affinities
 * P in CSR form (indptr N + 1 from 0, ids in [0, N), p finite and >= 0; N >= 2 is the index's size):
 *   q_ij = 1 / (1 + |y_i - y_j|^2),  R_i = sum_{j != i} q_ij^2 (y_i - y_j),  Z = sum_i sum_{j != i} q_ij,
 *   A_i = sum_{j in row i} P_ij q_ij (y_i - y_j),  grad_i = 4 (exaggeration A_i - R_i / Z),
 *   kl = sum_{P_ij > 0} P_ij log(P_ij Z / q_ij)   (P without the exaggeration).
 * All N^2 pairs are formed in fp64 with IEEE division; the order of every addition is fixed (the header
 * comment of csrc/tsne_kernels.h), so the result is a function of (y, P, N, exaggeration) alone,
 * whatever trlda_docindex_set_tsne_tile says.  grad_out is N x 2, kl_out one value. */
int trlda_docindex_tsne_gradient(trlda_docindex *index, const int64_t *indptr, const int64_t *ids, const double *p,
                                 const double *y, double exaggeration, double *grad_out, double *kl_out);
/* num_iterations steps of gradient descent on y (in: the start, out: the map).  Iteration t uses
 * early_exaggeration and momentum0 while t < exaggeration_iterations, then 1 and momentum1; elementwise
 * same = (g > 0) == (v > 0), gain = same ? gain 0.8 : gain + 0.2, gain = max(gain, 0.01) (gains start at
 * 1, v at 0), v = momentum v - learning_rate gain g, y += v; then the column means of y, formed in a
 * fixed tree, are subtracted.  kl_out[t] is the KL divergence before update t.  The whole loop is
 * enqueued on the model's stream and waited for once. */
int trlda_docindex_tsne_run(trlda_docindex *index, const int64_t *indptr, const int64_t *ids, const double *p,
                            double *y /* N x 2 */, int num_iterations, int exaggeration_iterations,
                            double early_exaggeration, double learning_rate, double momentum0, double momentum1,
                            double *kl_out /* num_iterations */);

/* Topic prevalence against what the caller knows about the indexed documents (csrc/effects_kernels.h,
 * DESIGN.md 3.34): the weighted mean and variance of theta^ per group of a labelling, and the parts of
 * the least-squares regression of theta^ (N x K) on a design matrix.  theta^ is recovered from the stored
 * rows as trlda_docindex_topic_documents recovers it.  Every + - x / is one rounded fp64 operation and
 * nothing is atomic in floating point: two calls agree bitwise, whatever trlda_docindex_set_slab_rows
 * says and however the index was filled.  weights_host (N, or NULL: every weight 1, and no multiply by
 * it) holds finite values >= 0.  TRLDA_ERR_ARG, before anything is waited for, copied or launched: a NULL
 * index, input or required output, an empty index, G outside [1, TRLDA_CLUSTER_MAX_CLUSTERS - 1], P
 * outside [1, TRLDA_EFFECTS_MAX_COLUMNS (256)]; TRLDA_ERR_VALUE, likewise (checked on the host): a label
 * outside [-1, G), a weight that is negative or not finite, a design or coefficient value that is not
 * finite.  A failed call leaves its outputs untouched.  Nothing is drawn; the index, lambda, alpha, the
 * counters and the model's statistics are left alone; pending deferred statistics and stream lanes are
 * settled first; the temporaries, the uploaded design and weights among them, are the call's own.  Each
 * call runs on the model's stream and synchronises once.
 *
 * The groups.  labels_host (int32, N) holds values in [-1, G); -1 leaves a document out.  The ids are
 * sorted by label with the stable counting sort of trlda_docindex_cluster (the left-out documents take
 * the slot past the last group); a group's members are taken in chunks of 256 in ascending id, the terms
 * of a chunk are added one after the other from 0.0, the chunk sums in ascending order, then one
 * division:
 *   mean_out[k + K g]   S_gk / W_g,  S_gk = sum_{d in g} w_d theta^_dk,  W_g = sum w_d (wsum_out[g]; without
 *                       weights the member count); NaN where W_g = 0
 *   ss_out[k + K g]     sum_{d in g} (w_d q) q,  q = theta^_dk - mean_gk (unless NULL; no division)
 *   count_out[g]        the members of g (int64), whatever their weights
 * A group's column depends on its members' rows, their weights and K alone -- not on the other groups,
 * their numbering or G.  No reference counterpart. */
int trlda_docindex_group_moments(trlda_docindex *index, const int32_t *labels_host /* N */, int G,
                                 const double *weights_host /* N or NULL */, double *mean_out /* K x G */,
                                 double *wsum_out /* G */, int64_t *count_out /* G */,
                                 double *ss_out /* K x G, may be NULL */);
/* gram_out (P x P, bitwise symmetric) = Z^T W Z and cross_out (P x K row-major) = Z^T W Theta^ of the
 * design z_host (N x P row-major, one row per indexed document in id order; an intercept is a column of
 * ones the caller adds).  64 x 64 tiles on v_mfma_f64_16x16x4_f64: the left operand is w_d z_dp (one
 * multiply), the right one z_dq or theta^_dk; N is cut into chunks of rows (a function of (P, K, N)
 * alone, or what trlda_docindex_set_moment_chunk forces: results then agree within rounding), every
 * element of a chunk is one chain of MFMAs over ascending rows, and the chunks' partial sums are added
 * in ascending order.  No reference counterpart. */
int trlda_docindex_regress_products(trlda_docindex *index, const double *z_host /* N x P row-major */, int P,
                                    const double *weights_host /* N or NULL */, double *gram_out /* P x P */,
                                    double *cross_out /* P x K */);
/* rss_out[k] = sum_d w_d (theta^_dk - sum_p z_dp b_pk)^2 with the coefficients coef_host (K rows of P:
 * b_pk at [k * P + p]), formed explicitly: fit is one chain of ceil(P / 4) MFMAs from +0 per (document,
 * topic) over ascending p, r = theta^ - fit, the term (w r) r; the terms of each fixed block of 64
 * documents are added in ascending document order from 0.0, the blocks in ascending order.  Nothing of
 * size N x K is written.  The total sum of squares about the weighted means is this call on the
 * one-column design of ones.  No reference counterpart. */
int trlda_docindex_regress_residuals(trlda_docindex *index, const double *z_host /* N x P row-major */, int P,
                                     const double *weights_host /* N or NULL */,
                                     const double *coef_host /* K x P row-major */, double *rss_out /* K */);

/* Indexed documents classified from their topic proportions (csrc/classify_kernels.h):
 * the device's part of the multinomial logistic regression of a label y_d in [0, C) on theta^_d, and its
 * predictions.  theta^ is recovered from the stored rows as trlda_docindex_topic_documents recovers it.
 * With the coefficients W (C x K row-major; no separate intercept, since sum_k theta^_dk = 1):
 *   z_dc = sum_k theta^_dk W_ck      one chain of ceil(K / 4) MFMAs from +0 over ascending k
 *   m = max_c z_dc,  e_c = exp(z_dc - m),  S = the e_c added one after the other from 0.0 in ascending c
 *   l_d = (log S + m) - z_{d,y_d},   p_dc = e_c / S,   r_dc = w_d (p_dc - [c = y_d])
 * Every + - x / is one rounded fp64 operation and nothing is atomic: two calls agree bitwise, however the
 * index was filled.  2 <= C <= TRLDA_CLASSIFY_MAX_CLASSES (128).  TRLDA_ERR_ARG, before anything is waited
 * for, copied or launched: a NULL index, input or required output, an empty index, C outside its range,
 * ids together with a gamma, an evaluation without labels or after the index has grown; TRLDA_ERR_VALUE,
 * likewise (checked on the host): a label outside [-1, C), a weight that is negative or not finite, a
 * coefficient that is not finite, an id outside the index, a gamma that is not finite and positive.  A
 * failed call leaves its outputs untouched.  Nothing is drawn; the index's rows, lambda, alpha, the
 * counters and the model's statistics are left alone.  Each call runs on the model's stream and
 * synchronises once.
 *
 * The labels of a fit go to the device once: labels_host (int32, N; -1 leaves a document out) and
 * weights_host (N finite values >= 0, or NULL: every weight 1 and no multiply by it) are uploaded and
 * kept on the index handle with the scratch of the evaluations until trlda_docindex_classify_clear, the
 * next trlda_docindex_classify_set or trlda_docindex_destroy.  weight_sum_out[0] = the weights of the
 * labelled documents added in ascending id from 0.0 on the host; count_out[c] the members of class c
 * (int64), whatever their weights.  No reference counterpart. */
int trlda_docindex_classify_set(trlda_docindex *index, const int32_t *labels_host /* N */, int C,
                                const double *weights_host /* N or NULL */, double *weight_sum_out /* 1 */,
                                int64_t *count_out /* C */);
/* Frees what trlda_docindex_classify_set keeps (nothing, if nothing is kept).  No reference counterpart. */
int trlda_docindex_classify_clear(trlda_docindex *index);
/* loss_out[0] = sum_d w_d l_d and grad_out (C x K row-major) = sum_d r_dc theta^_dk over the labelled
 * documents, unnormalised and without a penalty, for the labels that are set.  A workgroup owns a fixed
 * block of 64 documents: its terms w_d l_d are added in ascending document order from 0.0, the blocks in
 * ascending order.  The rows r (N x ceil(C / 4) * 4, the tail zero; a left-out document's row is exact
 * zeros) are written for a slab of rows at a time and contracted with theta^ by the cross items of
 * trlda_docindex_regress_products' kernel: chunks of rows (a function of (C, K, N) alone), every element
 * of a chunk one chain of MFMAs over ascending rows, the chunks' partial sums added in ascending order
 * once all slabs are done.  Neither sum depends on the slab or on the documents left out.  Up: C x K
 * doubles; down: 1 + C x K.  No reference counterpart. */
int trlda_docindex_classify_eval(trlda_docindex *index, const double *coef_host /* C x K row-major */,
                                 double *loss_out /* 1 */, double *grad_out /* C x K row-major */);
/* labels_out[i] (int32) = the first class of largest z for scored document i, and unless NULL
 * proba_out[i * C + c] = p_ic.  Scored are the M documents of ids_host (int64 row ids, any order, repeats
 * allowed), or the M columns of gamma_host (K x M, turned into rows as trlda_docindex_add_gamma turns
 * them: an indexed document and its gamma give the same bits), or with both NULL every indexed document
 * (M is ignored).  Needs no labels.  No reference counterpart. */
int trlda_docindex_classify_predict(trlda_docindex *index, const double *coef_host /* C x K row-major */, int C,
                                    const double *gamma_host /* K x M or NULL */, int64_t M,
                                    const int64_t *ids_host /* M or NULL */, int32_t *labels_out /* M or N */,
                                    double *proba_out /* (M or N) x C, may be NULL */);
/* A/B switch: rows of r per slab of trlda_docindex_classify_eval, rounded down to whole chunks and at
 * least one (0: what 256 MiB hold).  Results do not depend on it.  TRLDA_ERR_ARG while labels are set.
 * No reference counterpart. */
int trlda_docindex_set_classify_slab(trlda_docindex *index, int rows);

/* The words a document most likely holds next (csrc/recommend_kernels.h).  An E-step
 * on the batch from gamma (K x B host, in: gamma0, out: gamma; max_iter, threshold as for
 * trlda_model_estep_host), then per document d and word w of the vocabulary
 *   s(d, w) = sum_k (gamma_dk / sum_j gamma_dj) / rs_k * lambda_kw,  rs_k = sum_v lambda_kv,
 * which is p(w | d) under the point estimates of trlda_model_predictive, formed on the matrix cores
 * from lambda where it lies (no B x V matrix and no copy of lambda exist).  words_out (int32) and
 * probs_out (fp64), host, B x top_n row-major: per document the first top_n words in the total order
 * (s descending, word id ascending) and their s.  With exclude_seen != 0 the words document d has
 * seen -- an entry (w, c) with c > 0, the rule of trlda_cooc_add; repeated entries count once,
 * c <= 0 does not count -- are left out of its ranking; a document with fewer than top_n candidates
 * pads its row with (-1, 0.0).  A document without entries is ranked from its gamma like any other;
 * an empty batch writes nothing.  s depends on gamma_d, column w of lambda, the row sums and K alone:
 * a document's row is bitwise the same alone and inside any batch, whatever the slab width, and two
 * calls agree bitwise (the only atomics are the ORs that set the seen bits).
 * TRLDA_ERR_ARG, before anything is waited for, copied or launched: K above TRLDA_VI_MAX_TOPICS,
 * top_n outside [1, min(V, 100)], a batch of another V or device.  lambda, alpha and the counters are
 * left alone; pending deferred statistics and stream lanes are settled first; afterwards
 * trlda_model_get_sstats holds that E-step's statistics, as after trlda_model_word_topics.
 * Synchronises.  No reference counterpart. */
int trlda_model_recommend(trlda_model *model, const trlda_batch *batch, double *gamma, int top_n,
                          int exclude_seen, int max_iter, double threshold, int32_t *words_out,
                          double *probs_out);
/* The same rows from B gamma columns the caller keeps on the device (K x B, read only, not validated;
 * any K >= 1): no E-step runs, nothing is drawn, the model's statistics keep what they held.  With a
 * batch, which must hold B documents (else TRLDA_ERR_SHAPE), its seen words are left out; with NULL
 * every word is ranked.  words_dev / probs_dev: device arrays of B x top_n elements.  The same checks
 * otherwise.  Enqueued on the model's stream; does not synchronise.  On the same gamma bitwise the
 * rows of trlda_model_recommend.  No reference counterpart. */
int trlda_model_recommend_dev(trlda_model *model, const trlda_batch *batch_or_null, const double *gamma_dev,
                              int B, int top_n, int32_t *words_dev, double *probs_dev);
/* A/B switch for tests and measurements: words per workgroup of the ranking (a positive multiple of
 * 16; 0: the default, 2048).  The results do not depend on it.  No reference counterpart. */
int trlda_model_set_recommend_slab_words(trlda_model *model, int words);

/* Where held-out words stand in the ranking of the whole vocabulary (csrc/ranks_kernels.h, DESIGN.md
 * 3.30).  An E-step on observed_batch from gamma exactly as trlda_model_recommend runs it, then for
 * every entry p = (h, c) of heldout_batch, in its stored order, of document d
 *   ranks_out[p] = 1 + #{ w in [0, V) : w != h, w not seen by d, (s(d, w), w) before (s(d, h), h) },
 * s and the order (s descending, word id ascending) those of trlda_model_recommend: the 1-based
 * position of h in the list that call would return for d were top_n unbounded.  ranks_out[p] is 0
 * where the entry is no candidate (c <= 0, or with exclude_seen != 0 a word the observed document
 * has seen); a word listed twice gets its rank twice.  scores_out_or_null[p]: s(d, h), the bits
 * trlda_model_recommend returns for that pair, 0.0 where the rank is 0.  candidates_out[d] = V - (distinct
 * words d has seen), the length of d's ranking (V with exclude_seen == 0).  ranks_out (int32) and
 * scores_out (fp64) hold nnz(heldout_batch) elements, candidates_out (int32) B, all host.  The rank is a
 * count, taken behind the product trlda_model_recommend forms: no sort, no list, nothing of size B x V.
 * It depends on gamma_d, lambda, the row sums, K and d's seen words alone -- not on the batch, the
 * slab width or the threshold chunk --, and two calls agree bitwise (the only atomics are integer ORs
 * and adds).  TRLDA_ERR_ARG, before anything is waited for, drawn, copied or launched: K above
 * TRLDA_VI_MAX_TOPICS, a batch of another V or device, a NULL argument; TRLDA_ERR_SHAPE: the batches
 * hold different numbers of documents.  lambda, alpha and the counters are left alone; afterwards
 * trlda_model_get_sstats holds that E-step's statistics.  Synchronises.  No reference counterpart. */
int trlda_model_heldout_ranks(trlda_model *model, const trlda_batch *observed_batch,
                              const trlda_batch *heldout_batch, double *gamma, int exclude_seen, int max_iter,
                              double threshold, int32_t *ranks_out, double *scores_out_or_null,
                              int32_t *candidates_out);
/* The same from B gamma columns the caller keeps on the device (K x B, read only, not validated; any
 * K >= 1): no E-step runs, nothing is drawn, the model's statistics keep what they held.  Both batches
 * must hold B documents (else TRLDA_ERR_SHAPE); with observed_batch NULL every word is a candidate.
 * ranks_dev / scores_dev_or_null (nnz(heldout_batch)) and candidates_dev (B): device arrays.  Enqueued
 * on the model's stream; does not synchronise.  On the same gamma bitwise the results of
 * trlda_model_heldout_ranks.  No reference counterpart. */
int trlda_model_heldout_ranks_dev(trlda_model *model, const trlda_batch *observed_batch_or_null,
                                  const trlda_batch *heldout_batch, const double *gamma_dev, int B,
                                  int32_t *ranks_dev, double *scores_dev_or_null, int32_t *candidates_dev);
/* A/B switch for tests: how many of a document's thresholds (held-out entries) one counting sweep
 * holds (1 ... 32; 0: the default, 32); a document with more takes further sweeps over the same
 * words.  The results do not depend on it.  The slab of words is that of
 * trlda_model_set_recommend_slab_words.  No reference counterpart. */
int trlda_model_set_ranks_chunk(trlda_model *model, int pairs);

/* Topic words by relevance, corpus terms by saliency, and the topic prevalence of a corpus
 * (csrc/relevance_kernels.h).  With R_k = sum_w lambda_kw and topic weights pi
 * (topic_weights == NULL: pi_k = R_k / sum_j R_j; else K host values, finite and > 0, normalised to
 * sum 1 on the host):
 *   p_w = sum_k c_k lambda_kw, c_k = pi_k / R_k          the marginal word probability
 *   r_kw = log lambda_kw - log R_k - (1 - weight) log p_w  relevance (Sievert & Shirley 2014)
 *   D_w = sum_k q_kw (log q_kw - log pi_k), q_kw = c_k lambda_kw / p_w   distinctiveness, KL(p(k|w) || pi)
 *   S_w = p_w D_w                                        saliency (Chuang, Manning & Heer 2012)
 * The sums over k run in an order that depends on K alone, the row sums in an order that depends on K
 * and V; no atomics: every result repeats bitwise.  A lambda with an element <= 0 or not finite fails
 * each of the three calls with TRLDA_ERR_VALUE ("relevance needs a positive, finite lambda") and
 * nothing is written to the outputs.  TRLDA_ERR_ARG, before anything is allocated or launched: a NULL
 * output, a weight that is not finite or <= 0, top_n outside [1, min(V, 100)], weight outside [0, 1].
 * lambda, alpha, the counters, the statistics and the seeded stream are left alone; pending deferred
 * statistics and stream lanes are settled first.  Each call synchronises.  No reference counterpart. */

/* p_out, distinct_out, saliency_out (V each, host) = p_w, D_w, S_w. */
int trlda_model_word_stats(trlda_model *model, const double *topic_weights, double *p_out,
                           double *distinct_out, double *saliency_out);
/* words_out (K x top_n int32, host, topic-major: [k * top_n + r]) = the top_n word ids of each topic
 * in decreasing r_kw, equal values by smaller id first -- np.lexsort((arange(V), -r[k]))[:top_n], the
 * tie rule of trlda_model_top_words, whose order weight = 1 reproduces wherever log keeps distinct
 * lambda apart; scores_out (K x top_n fp64, or NULL) = their r_kw. */
int trlda_model_relevant_words(trlda_model *model, int top_n, double weight, const double *topic_weights,
                               int32_t *words_out, double *scores_out);
/* words_out (top_n int32, host) = the top_n word ids in decreasing S_w, equal values by smaller id
 * first; saliency_out (top_n fp64, or NULL) = their S_w. */
int trlda_model_salient_words(trlda_model *model, int top_n, const double *topic_weights,
                              int32_t *words_out, double *saliency_out);

/* The words nearest a word in topic space (csrc/wordsim_kernels.h).  With R_k, pi and
 * c_k = pi_k / R_k as above (topic_weights: NULL or K host values, the rule of
 * trlda_model_relevant_words), a_kw = c_k lambda_kw and p(k | w) = a_kw / sum_j a_jw, word w has the row
 *   measure 0 (hellinger):  r_wk = sqrt(p(k | w))                 s = the Bhattacharyya coefficient
 *   measure 1 (cosine):     r_wk = a_kw / sqrt(sum_j a_jw^2)      s = the cosine
 * and s(q, w) = sum_k r_qk r_wk -- the two measures of trlda_docindex_create -- formed on the matrix
 * cores from lambda where it lies: no V x K table of rows and no copy of lambda exist.  words_out
 * (int32) and sim_out (fp64), host, B x top_n row-major: per query the first top_n words in the total
 * order (s descending, word id ascending) and their s.  s(q, w) depends on columns q and w of lambda,
 * on c and on K alone: a query's row is bitwise the same alone and inside any batch, whatever the slab
 * width; s(q, w) and s(w, q) are the same bits; two calls agree bitwise (no atomics).
 * TRLDA_ERR_ARG, before anything is allocated or launched: a NULL model or output, B < 0, top_n outside
 * [1, min(V - e, 100)] (e = 1 with exclude_self, else 0), a measure that is not 0 or 1, a weight that
 * is not finite or <= 0; then TRLDA_ERR_WORD_ID for an id outside [0, V) and TRLDA_ERR_VALUE for
 * proportions that are not finite or not > 0.  A lambda with an element <= 0 or not finite fails with
 * TRLDA_ERR_VALUE ("word similarity needs a positive, finite lambda") and nothing is written to the
 * outputs.  B = 0 writes nothing.  lambda, alpha, the counters, the statistics and the seeded stream are
 * left alone, nothing is drawn; pending deferred statistics and stream lanes are settled first.  Each
 * call synchronises. */

/* The words nearest the B words word_ids (host).  With exclude_self != 0 the query word itself is left
 * out of its own ranking by id; another word with an equal column stays in, at s = 1 up to rounding.
 * No reference counterpart. */
int trlda_model_similar_words(trlda_model *model, const int32_t *word_ids /* B */, int B, int top_n,
                              int measure, const double *topic_weights /* K or NULL */, int exclude_self,
                              int32_t *words_out /* B x top_n */, double *sim_out /* B x top_n */);
/* The words nearest B points of the topic simplex: proportions (K x B fp64 host, finite and > 0,
 * normalised as trlda_docindex_query_gamma normalises gamma) -- a document's theta, a centroid of
 * trlda_docindex_cluster, a topic.  There is no self to leave out.  No reference counterpart. */
int trlda_model_similar_words_rows(trlda_model *model, const double *proportions /* K x B */, int B, int top_n,
                                   int measure, const double *topic_weights /* K or NULL */,
                                   int32_t *words_out /* B x top_n */, double *sim_out /* B x top_n */);
/* out (K x B fp64 host, column-major: [b * K + k]) = p(k | word_ids[b]), the quantity the measures
 * compare; its sum over k in the order of the ranking's column pass.  The errors of
 * trlda_model_similar_words that apply.  No reference counterpart. */
int trlda_model_word_topic_proportions(trlda_model *model, const int32_t *word_ids /* B */, int B,
                                       const double *topic_weights /* K or NULL */, double *out);
/* A/B switch for tests and measurements: words per workgroup of the ranking (a positive multiple of
 * 16; 0: the default, 2048).  The results do not depend on it.  No reference counterpart. */
int trlda_model_set_wordsim_slab_words(trlda_model *model, int words);

/* A prevalence accumulator for `model`: pi_k ~ sum_d N_d gamma_dk / sum_j gamma_dj over the documents
 * added, N_d = the sum of document d's positive counts (weight_by_length == 0: 1); a document without
 * a positive count is skipped.  K fp64 sums stay on the device between batches: one addition per
 * document per topic in the order the documents are added, each document's sum_j gamma_dj in an order
 * that depends on K alone, so the result is bitwise independent of how the documents are cut into
 * batches.  It runs on the model's stream and must be destroyed before the model. */
typedef struct trlda_prevalence trlda_prevalence;
int trlda_prevalence_create(trlda_model *model, int weight_by_length, trlda_prevalence **out);
/* An E-step on the batch as trlda_model_estep_host runs it (gamma: K x B host, in: gamma0, out:
 * gamma; afterwards trlda_model_get_sstats holds that E-step's statistics), then its documents are
 * added.  TRLDA_ERR_ARG, before anything is waited for, copied or launched: K above
 * TRLDA_VI_MAX_TOPICS, a batch of another V or device.  Synchronises. */
int trlda_prevalence_add(trlda_prevalence *prevalence, const trlda_batch *batch, double *gamma, int max_iter,
                         double threshold);
/* Adds the batch's documents with a gamma the caller keeps on the device (K x B, read only, not
 * validated; any K >= 1): no E-step runs, nothing is drawn.  Enqueued on the model's stream; does not
 * synchronise.  On the same gamma bitwise the sums of trlda_prevalence_add. */
int trlda_prevalence_add_dev(trlda_prevalence *prevalence, const trlda_batch *batch, const double *gamma_dev);
/* prevalence_out (K, host) = the sums so far normalised to sum 1 (on the host, one rounding each);
 * *num_docs = the documents that contributed.  None: TRLDA_ERR_VALUE.  Synchronises. */
int trlda_prevalence_read(trlda_prevalence *prevalence, double *prevalence_out, int64_t *num_docs);
int trlda_prevalence_destroy(trlda_prevalence *prevalence);

/* Per-topic quality diagnostics (csrc/diagnostics_kernels.h).  With R_k, pi and p_w as
 * for trlda_model_word_stats, beta_kw = lambda_kw (1 / R_k) and log beta_kw = log lambda_kw - log R_k,
 * K host values each:
 *   eff_out         1 / sum_w beta_kw^2                           the effective number of words
 *   entropy_out     H_k = -sum_w beta_kw log beta_kw
 *   uniform_out     log V - H_k = KL(beta_k || uniform), formed on the host from H_k
 *   corpus_out      sum_w beta_kw (log beta_kw - log p_w) = KL(beta_k || p)
 *   exclusivity_out the mean over r < top_n, in rank order, of beta_kw / sum_j beta_jw, w = words[k * top_n + r]
 * words (K x top_n int32, host, topic-major) are the lists the exclusivity is averaged over, e.g. those
 * of trlda_model_top_words or trlda_model_relevant_words.  The sums over w run over chunks of 256
 * consecutive words, ascending inside a chunk and then over the chunks, the sums over j in an order that
 * depends on K alone; no atomics: every result repeats bitwise.  K = 1 gives exclusivity exactly 1.
 * TRLDA_ERR_ARG, before anything is allocated or launched: a NULL argument, top_n outside
 * [1, min(V, 100)], a weight that is not finite or <= 0, a word twice in a list; TRLDA_ERR_WORD_ID: an
 * id outside [0, V).  A lambda with an element <= 0 or not finite fails with TRLDA_ERR_VALUE ("topic
 * diagnostics needs a positive, finite lambda") and nothing is written to the outputs.  lambda, alpha,
 * the counters, the statistics and the seeded stream are left alone; pending deferred statistics and
 * stream lanes are settled first.  Synchronises.  No reference counterpart. */
int trlda_model_word_diagnostics(trlda_model *model, int top_n, const double *topic_weights /* K or NULL */,
                                 const int32_t *words /* K x top_n */, double *eff_out, double *entropy_out,
                                 double *uniform_out, double *corpus_out, double *exclusivity_out);

/* The document side's accumulator for `model`, in the mould of trlda_prevalence (N_d, the skipped
 * documents and sum_j gamma_dj as there).  Per contributing document a_dk = (N_d gamma_dk) / sum_j
 * gamma_dj and theta_dk = gamma_dk / sum_j gamma_dj; kept on the device between batches: T_k = sum_d
 * a_dk (bitwise the sums behind trlda_prevalence_read on the same gamma), A_k = sum_d a_dk log a_dk,
 * and the int64 counts of the documents whose largest gamma_dj is j = k (ties to the smaller j), with
 * theta_dk > high, and with theta_dk > low.  One addition per document per sum in the order the
 * documents are added: bitwise independent of how they are cut into batches.  0 <= low < high < 1,
 * else TRLDA_ERR_ARG before anything is allocated.  It runs on the model's stream and must be
 * destroyed before the model.  No reference counterpart. */
typedef struct trlda_topicdiag trlda_topicdiag;
int trlda_topicdiag_create(trlda_model *model, int weight_by_length, double high, double low,
                           trlda_topicdiag **out);
/* trlda_prevalence_add's E-step on the batch (gamma: K x B host, in: gamma0, out: gamma), then its
 * documents are added; the same errors.  Synchronises. */
int trlda_topicdiag_add(trlda_topicdiag *diag, const trlda_batch *batch, double *gamma, int max_iter,
                        double threshold);
/* Adds the batch's documents with a gamma the caller keeps on the device (K x B, read only, not
 * validated; any K >= 1): no E-step runs, nothing is drawn.  Does not synchronise. */
int trlda_topicdiag_add_dev(trlda_topicdiag *diag, const trlda_batch *batch, const double *gamma_dev);
/* K host values each: tokens_out = T_k; entropy_out = log T_k - A_k / T_k, the entropy of p(d | k) =
 * a_dk / T_k (closed in long double on the host); rank1_out, high_out, low_out = the counts;
 * *num_docs = the documents that contributed.  None: TRLDA_ERR_VALUE.  Synchronises. */
int trlda_topicdiag_read(trlda_topicdiag *diag, double *tokens_out, double *entropy_out, int64_t *rank1_out,
                         int64_t *high_out, int64_t *low_out, int64_t *num_docs);
int trlda_topicdiag_destroy(trlda_topicdiag *diag);

/* Distances between topics (csrc/topicdist_kernels.h).  A topic is p_i = lambda_i /
 * S_i, S_i = sum_v lambda_iv; the second lambda, mu (K2 x V), gives q_j = mu_j / T_j.  dist_out (K x K2
 * column-major, host: [i + K * j]) =
 *   TRLDA_TOPICDIST_HELLINGER  sqrt(max(0, 1 - sum_v sqrt(p_iv q_jv)))
 *   TRLDA_TOPICDIST_COSINE     max(0, 1 - sum_v p_iv q_jv / (|p_i| |q_j|))
 *   TRLDA_TOPICDIST_KL         sum_v p_iv log(p_iv / q_jv), nats, the row topic first
 *   TRLDA_TOPICDIST_JS         H(m) - H(p_i) / 2 - H(q_j) / 2, m = (p_i + q_j) / 2, nats (not its root)
 * The second lambda is `other`'s (a model of the same V on the same device), or lambda_host (K2 x V
 * column-major, uploaded to a temporary and not kept; not validated), or with both NULL -- or
 * other == model -- the model's own: then the diagonal is exactly 0 and the three symmetric measures
 * are bitwise symmetric.  K2 is the second lambda's number of topics in every case.  No floating-point
 * atomics: how V is cut into chunks and the matrix into tiles depends on (K, K2, V, measure) alone and
 * the chunks' sums are added in ascending order, so equal inputs give equal bits.  A lambda with zeros
 * gives what IEEE arithmetic gives.
 * TRLDA_ERR_ARG, before anything is waited for, copied or launched: a NULL model or dist_out, both
 * `other` and lambda_host, another V or device, a K2 that is not the second lambda's, an unknown
 * measure, more tiles or chunks than a grid takes.  Runs on the model's stream; pending deferred
 * statistics and stream lanes of both models are settled first and `other`'s stream is waited for.
 * lambda, alpha and the generator are left alone.  Synchronises.  No reference counterpart. */
#define TRLDA_TOPICDIST_HELLINGER 0
#define TRLDA_TOPICDIST_COSINE    1
#define TRLDA_TOPICDIST_KL        2
#define TRLDA_TOPICDIST_JS        3
int trlda_model_topic_distances(trlda_model *model, trlda_model *other, const double *lambda_host, int K2,
                                int measure, double *dist_out);
/* A/B switch for tests and measurements: words per chunk of V in trlda_model_topic_distances (any
 * positive number; 0: automatic).  The results agree within rounding, not bitwise.  No reference
 * counterpart. */
int trlda_model_set_topicdist_chunk(trlda_model *model, int words);

/* LDA::updateVariablesGibbs (src/lda.cpp:224-293), reached from python/src/ldainterface.cpp:311-390
 * with inference_method='GIBBS': collapsed Gibbs sampling of the batch's topic assignments on the
 * device (csrc/gibbs_kernels.h), one wave64 per document, K <= 1024 (more: TRLDA_ERR_ARG).
 *   theta0_dev  K x B initial theta (lda.cpp:229-230), or NULL: Dirichlet(1) per column drawn from
 *               the key (lda.cpp:123-128 draws sampleDirichlet from the host stream)
 *   theta_dev   out: K x B, Dirichlet(alpha + topic counts) of the final state (lda.cpp:288)
 *   sstats_dev  out: K x V, tokens per (topic, word) summed over the num_samples sweeps after
 *               burn_in, times 1 / num_samples (lda.cpp:278-284; not multiplied by exp E[log beta])
 *   key         the 64-bit Philox4x32-10 key: every draw is a function of (key, document index,
 *               token or topic, sweep, purpose) -- the counter layout is pinned in gibbs_kernels.h
 * Deviations from the reference: the init reads theta0's column i, not j
 * (lda.cpp:254); Philox instead of rand() / mt19937; sstats as exact counts scaled once;
 * Marsaglia-Tsang gamma draws in log space for theta.  A histogram that sums to 0 or is not
 * finite fails the call with "Something went wrong while sampling from histogram."
 * (utils.cpp:198).  num_samples or burn_in < 0: TRLDA_ERR_ARG.  Flushes the deferred work first
 * and uses workspaces of its own: trlda_model_get_sstats, the deferred statistics, the lanes and
 * the prefetch announcements keep what they held for the VI path.  Those workspaces -- the K x V
 * double table, K x V uint32 counts, a uint16 per token of the largest batch so far (and, for
 * trlda_model_gibbs_host, K x B and K x V double staging) -- stay allocated after the first Gibbs
 * call until trlda_model_destroy: about 1 GB at K = 500, V = 100 000.  Synchronises. */
int trlda_model_gibbs(trlda_model *model, const trlda_batch *batch, const double *theta0_dev,
                      double *theta_dev, double *sstats_dev, int num_samples, int burn_in,
                      uint64_t key);

/* Host-pointer convenience around trlda_model_gibbs: theta (K x B host) is the initial theta when
 * use_latents != 0 (else Dirichlet(1) is drawn on the device) and receives the sampled theta;
 * sstats (K x V host) receives the statistics.  The key is the next two draws of the library's
 * libc-compatible stream (first draw: low 32 bits).  Those draws are rand()'s 31-bit values, so
 * bits 31 and 63 of the key are always 0: 62 bits vary.  trlda_seed() makes a call reproducible and
 * successive calls differ.  src/lda.cpp:224-293, python/src/ldainterface.cpp:311-390. */
int trlda_model_gibbs_host(trlda_model *model, const trlda_batch *batch, double *theta, int use_latents,
                           double *sstats, int num_samples, int burn_in);

/* Collapsed variational Bayes, zero order (CVB0) of the batch's documents on the model's fixed
 * topics, on the device (csrc/cvb0_kernels.h, whose header is the contract), one wave64 per
 * document, K <= 1024 (more: TRLDA_ERR_ARG before anything is allocated or launched).  No reference
 * counterpart: Asuncion, Welling, Smyth & Teh, "On smoothing and inference for topic models" (UAI
 * 2009), with the document-side update of Foulds, Boyles, DuBois, Smyth & Welling, "Stochastic
 * collapsed variational Bayesian inference for latent Dirichlet allocation" (KDD 2013).  It is the
 * deterministic form of the conditional trlda_model_gibbs samples from,
 * phi_ik ~ (alpha_k + sum_{j != i} phi_jk) e[k, w_i], on the Gibbs path's normalised table e
 * (trlda_debug_gibbs_table returns what the call read).
 *   theta0_dev  K x B, the weights the documents' phi start from (phi_p ~ theta0 e[:, w_p]), or
 *               NULL: alpha
 *   theta_dev   out: K x B, (alpha + n) / (sum alpha + N_d), n the expected topic counts
 *   sstats_dev  out: K x V, expected tokens per (topic, word), sum over the word's entries of
 *               c_p phi_p in document order; not multiplied by exp E[log beta]; 0 outside the batch
 *   max_iter    Gauss-Seidel sweeps over a document's entries, at most (0: the init state)
 *   threshold   a document stops after the sweep whose mean |change of n| is below it (0: never)
 *   iters_dev   out, or NULL: B sweeps done per document
 * One phi per entry (word type) with a ONE-token self-exclusion.  No random numbers (the library's
 * stream is not advanced), no atomics: two calls give bitwise the same result, whatever the launch
 * geometry, the lanes or the slab cap.  A token whose weights sum to 0 or are not finite fails the
 * call with TRLDA_ERR_VALUE.  max_iter < 0: TRLDA_ERR_ARG.  Flushes the deferred work first and
 * touches none of the VI path's state: trlda_model_get_sstats, the deferred statistics, the lanes
 * and the prefetch announcements keep what they held.  Workspaces -- the Gibbs path's K x V table,
 * phi as entries x K doubles of a slab (trlda_model_set_cvb0_slab_bytes), two int32 per entry and
 * document -- stay allocated until trlda_model_destroy.  Synchronises. */
int trlda_model_cvb0(trlda_model *model, const trlda_batch *batch, const double *theta0_dev,
                     double *theta_dev, double *sstats_dev, int max_iter, double threshold,
                     int32_t *iters_dev);

/* Host-pointer convenience around trlda_model_cvb0: theta (K x B host) holds theta0 when
 * use_latents != 0 and receives theta; sstats (K x V host) and iters (B host, or NULL) receive the
 * statistics and the sweeps done.  Staged through trlda_model_gibbs_host's buffers.  No reference
 * counterpart (Asuncion et al. 2009; Foulds et al. 2013). */
int trlda_model_cvb0_host(trlda_model *model, const trlda_batch *batch, double *theta, int use_latents,
                          double *sstats, int max_iter, double threshold, int32_t *iters);

/* A/B switch for tests: the cap in bytes on trlda_model_cvb0's phi scratch (0: the default, 1 GiB
 * -- a chosen number, not a measured one).  The batch's documents are worked off in slabs, in batch
 * order, whose entries x K doubles fit the cap (a document that alone exceeds it is a slab of its
 * own); results are bitwise independent of it.  No reference counterpart. */
int trlda_model_set_cvb0_slab_bytes(trlda_model *model, size_t bytes);

/* ---- sampling documents: LDA::sample, src/lda.cpp:88-115, python/src/ldainterface.cpp:218-262 ----
 * Topics beta_k ~ Dirichlet(lambda_k) are drawn once per call; per document d, its length
 * n_d ~ Poisson(length), theta_d ~ Dirichlet(alpha) and, per token, a topic z ~ theta_d and a
 * word w ~ beta_z.  A document is its word ids in token order (every count is 1; repeats are
 * allowed).  Every draw is Philox4x32-10 of a 64-bit key and a counter pinned in csrc/philox.h
 * (purposes 8 - 15), so nothing depends on the launch, the device or B: with one key, the first n
 * documents of B > n are the n documents of B = n.  Deviations from the reference (DESIGN.md
 * 3.11): Philox instead of rand(), Poisson by inversion (utils.cpp:269-287's product method fails
 * from length 745 on), O(log V) word draws by binary search in a prefix table.
 *
 * The key for the host entries: the next two draws of the library's libc-compatible stream (first
 * draw: the low 32 bits; 62 bits vary), the same as trlda_model_gibbs_host's.  A gamma0 drawn ahead
 * by a model is given back to the stream first.  trlda_seed() makes a sequence of calls
 * reproducible; successive calls differ. */
int trlda_rng_draw_key(uint64_t *key);

/* The B lengths (purpose 14, counter (d, 0, 0); u in [0, 1)) as CSR offsets: indptr_out[B+1],
 * indptr_out[0] = 0.  n_d inverts Poisson(length) against a table built with log, exp and
 * sequential sums only: l_0 = -length, l_k = l_{k-1} + log(length) - log(k), pmf_k = exp(l_k),
 * CDF_k = CDF_{k-1} + pmf_k up to k_max = ceil(length + 12 sqrt(length) + 40); n_d is the first k
 * with CDF_k > u * CDF_kmax, or, when u * CDF_kmax rounds up to CDF_kmax, the first k whose CDF
 * equals CDF_kmax.  length = 0: every document is empty.  TRLDA_ERR_ARG: length < 0 or not finite,
 * B < 0, or a total (indptr_out[B]) that does not fit in int32.  Host only: no device needed. */
int trlda_sample_lengths(int B, double length, uint64_t key, int32_t *indptr_out);

/* The documents on the device: indptr_dev (B+1, from trlda_sample_lengths; trusted as given) in,
 * ids_dev (indptr[B] int32 word ids) out, theta_dev (K x B, the documents' theta) out unless NULL.
 * Reads lambda and alpha only; flushes the deferred work and the lanes first.  The VI workspaces,
 * trlda_model_get_sstats, the announcements and the Gibbs state keep what they held.  A topic row
 * or theta whose weights do not sum to a finite number > 0 (an all-zero lambda row when eta = 0,
 * say) fails the call with "Something went wrong while sampling from histogram." (utils.cpp:198).
 * Workspaces, allocated on first use and kept until trlda_model_destroy (hipFree synchronises the
 * device): the K x V double prefix table (K * V * 8 bytes, 400 MB at K = 500, V = 100 000;
 * shared with the Gibbs path's table), 2 x K x ceil(V / 4096) doubles of chunk totals, and a
 * K x B double prefix scratch sized to the largest B so far (for trlda_model_sample_host also
 * B+1 and nnz int32 and K x B double staging).  Synchronises. */
int trlda_model_sample(trlda_model *model, int B, const int32_t *indptr_dev, int32_t *ids_dev,
                       double *theta_dev, uint64_t key);

/* Host-pointer form of trlda_model_sample: indptr (B+1 host; checked: starts at 0, never
 * falls) in, ids (indptr[B] host) and theta (K x B host, or NULL) out, staged through buffers the
 * model holds.  python/src/ldainterface.cpp:218-262 -> src/lda.cpp:88-115. */
int trlda_model_sample_host(trlda_model *model, int B, const int32_t *indptr, int32_t *ids,
                            double *theta, uint64_t key);

/* ---- the utilities of trlda.utils (python/utils/__init__.py) ------------------------------- */

/* TRLDA::polygamma(int, double), src/utils.cpp:107-111: psi(x) for n < 1, (-1)^(n+1) n! zeta(n+1, x)
 * for n >= 1 (csrc/polygamma.h).  A non-positive integer x gives +inf for the zeta, so +inf for psi
 * and odd n, -inf for even n >= 2; x = +inf gives +inf (n < 1) or a signed 0; nan gives nan; for n >= 1
 * a non-integer x below -2^20 gives nan.  Host only: no device needed.  The same function as a device
 * element of trlda_polygamma_device, to the last bit. */
double trlda_polygamma(int n, double x);

/* TRLDA::polygamma(int, const ArrayXXd&), src/utils.cpp:115-123: y_dev[i] = polygamma(n, x_dev[i]),
 * i < count, device pointers on `device` (in place allowed), on the null stream; synchronises. */
int trlda_polygamma_device(int n, int64_t count, const double *x_dev, double *y_dev, int device);

/* Host-pointer form of trlda_polygamma_device, staged through a device buffer
 * (python/src/utilsinterface.cpp, polygamma on an array). */
int trlda_polygamma_host(int n, int64_t count, const double *x, double *y, int device);

/* TRLDA::sampleDirichlet, src/utils.cpp:251-266: out_dev (m x n, F-order, a device pointer) gets n
 * columns, each a draw from Dirichlet(alpha 1_m) (csrc/dirichlet_kernels.h): Philox under `key`,
 * purposes 16 / 17 / 18, counter (row, column, attempt); a summation order that depends on m only.
 * TRLDA_ERR_ARG: m or n < 0, alpha not > 0 or not finite.  m = 0 or n = 0: nothing is written.
 * Null stream; synchronises. */
int trlda_sample_dirichlet_device(int m, int n, double alpha, uint64_t key, double *out_dev, int device);

/* Host-pointer form (python/src/utilsinterface.cpp, sample_dirichlet): the key is
 * trlda_rng_draw_key()'s, drawn by every call that passes the argument checks (also for m = 0 or
 * n = 0, which need no device); out (m x n, F-order) is staged through a device buffer. */
int trlda_sample_dirichlet_host(int m, int n, double alpha, double *out, int device);

/* TRLDA::randomSelect, src/utils.cpp:351-378: k of 0 .. n-1, drawn with rand() % n from the seeded
 * stream exactly as the reference draws them (a gamma0 drawn ahead is given back first); out[0 .. k)
 * gets them in ascending order.  TRLDA_ERR_ARG "k must be smaller than n." (k > n), then "n and k must
 * be non-negative.".  Host only. */
int trlda_random_select(int k, int n, int32_t *out);

/* model.lambda = (1-rho) lambda' + rho (eta + scale * sstats), all device pointers.
 * src/onlinelda.cpp:99-100, :108-109; src/batchlda.cpp:60 (rho = 1, scale = 1). */
int trlda_model_blend(trlda_model *model, const double *lambda_prime_dev,
                      const double *sstats_dev, double rho, double eta, double scale);

/* model.lambda = (1-rho) lambda' (+row) rho (eta + D/B/K * wordcounts): src/onlinelda.cpp:79-86 */
int trlda_model_tr_init(trlda_model *model, const trlda_batch *batch,
                        const double *lambda_prime_dev, double rho, double eta,
                        int num_documents);

/* The two halves of trlda_model_tr_init, for the multi-GPU composition where the word
 * counts of the whole mini-batch are the sum over ranks (src/onlinelda.cpp:79-82 is a sum
 * over documents): local counts -> all-reduce -> apply.
 *   wordcounts_dev  V fp64 (integer-valued, so the sum is exact in any order)
 *   coef            D / B_total / K, evaluated by the caller in that order (onlinelda.cpp:86) */
int trlda_model_wordcounts(trlda_model *model, const trlda_batch *batch, double *wordcounts_dev);
int trlda_model_tr_init_wc(trlda_model *model, const double *wordcounts_dev,
                           const double *lambda_prime_dev, double rho, double eta, double coef);

/* dst_dev[K x V] = model.lambda (device-to-device, on the model's stream): the
 * `lambdaPrime = mLambda` snapshot of src/onlinelda.cpp:68. */
int trlda_model_copy_lambda(trlda_model *model, double *dst_dev);

/*
 * OnlineLDA::updateParameters, lambda path: src/onlinelda.cpp:53-111, 177-179 (the
 * caller of python/src/onlineldainterface.cpp:204-256).  Runs the whole
 * trust-region loop on the device; gamma initial values are drawn on the host from
 * libc rand() at exactly the points the reference draws them (src/lda.cpp:135) so
 * trlda_seed() pins the trajectory.  threshold is the reference's fixed 0.001
 * unless overridden.  Returns rho through *rho_out and increments *update_count
 * (not for an empty batch: src/onlinelda.cpp:54-56, which returns 1.0).
 *   gamma_out  optional host K x B: gamma of the last E-step
 * Single GPU.  The multi-GPU composition (E-step -> RCCL all-reduce of sstats ->
 * blend) is done by the host mirror from the three calls above.
 * Returns without waiting for the device unless gamma_out is given (every getter
 * synchronises): the host's draw of the next gamma0 overlaps this call's kernels.
 */
int trlda_model_online_update(trlda_model *model, const trlda_batch *batch,
                              int num_documents, double eta,
                              int max_iter_tr, int max_iter_inference,
                              double kappa, double tau, double rho,
                              int init_gamma, int update_lambda, double threshold,
                              int *update_count, double *rho_out, double *gamma_out);

/*
 * BatchLDA::updateParameters, lambda path: src/batchlda.cpp:43-61 -- max_epochs x
 * { E-step from a fresh random gamma; lambda = eta + sstats }.
 */
int trlda_model_batch_update(trlda_model *model, const trlda_batch *batch, double eta,
                             int max_epochs, int max_iter_inference, int update_lambda,
                             double threshold, double *gamma_out);

/*
 * OnlineLDA::updateParameters with inferenceMethod = GIBBS (src/onlinelda.cpp:53-179, its
 * E-steps through src/lda.cpp:119-157 -> 224-293; Mimno, Hoffman & Blei 2012): with
 * max_iter_tr > 0, the initial step from the word counts (:79-86), then max_iter_tr x
 * { Gibbs E-step; lambda = (1 - rho) lambda' + rho (eta + D / B sstats) } (:89-101); with
 * max_iter_tr = 0, one E-step on lambda as it is and the same blend (:103-109).  rho < 0: the
 * schedule (tau + update_count)^-kappa (:59-66).  init_theta != 0: every iteration after the first
 * starts from the previous iteration's theta, else from Dirichlet(1) (lda.cpp:123-128).
 * Each E-step is trlda_model_gibbs with the key of trlda_rng_draw_key, drawn in loop order after
 * every argument check (an error draws nothing and leaves lambda alone).  The loop runs on the
 * device without a wait (csrc/gibbs_kernels.h, gibbs_mstep_kernel): the words outside the batch
 * are written once per call, each iteration touches the batch's active words only.  With
 * trlda_model_set_keep_sstats on, the statistics (trlda_model_get_sstats) and the whole lambda'
 * stay behind for trlda_model_adaptive_stats.  K <= 1024, num_samples, burn_in >= 0 (else
 * TRLDA_ERR_ARG).  theta_out: optional host K x B, theta of the last E-step.  Inside the loop
 * nothing waits for the device; the call waits at its end (the sampler's failure flag), and before
 * the loop when the batch is not the one the model last made a Gibbs plan for (trlda_model_gibbs:
 * the token counts are downloaded and the plan uploaded, two waits -- once per new batch).  A
 * histogram that sums to 0 or is not finite fails the call with "Something went wrong while
 * sampling from histogram." (lambda is then already written).
 */
int trlda_model_online_update_gibbs(trlda_model *model, const trlda_batch *batch, int num_documents,
                                    double eta, int max_iter_tr, double kappa, double tau, double rho,
                                    int init_theta, int update_lambda, int num_samples, int burn_in,
                                    int *update_count, double *rho_out, double *theta_out);

/*
 * BatchLDA::updateParameters with inferenceMethod = GIBBS (src/batchlda.cpp:43-61): max_epochs x
 * { Gibbs E-step from a fresh Dirichlet(1) theta; lambda = eta + sstats }, as
 * trlda_model_online_update_gibbs does it (keys, checks, one wait).
 */
int trlda_model_batch_update_gibbs(trlda_model *model, const trlda_batch *batch, double eta,
                                   int max_epochs, int update_lambda, int num_samples, int burn_in,
                                   double *theta_out);

/*
 * CumulativeLDA::updateParameters, lambda path: src/cumulativelda.cpp:49-72 -- lambda' =
 * lambda; lambda = sampleGamma(K, V, 100)/100 (drawn whether or not update_lambda is set,
 * like the reference); max_epochs x { E-step from a fresh random gamma; lambda = lambda' +
 * sstats }.
 */
int trlda_model_cumulative_update(trlda_model *model, const trlda_batch *batch, int max_epochs,
                                  int max_iter_inference, int update_lambda, double threshold,
                                  double *gamma_out);

/* ---- multi-GPU: documents shard across ranks, one RCCL all-reduce per E-step ---------------
 *
 * One process per GPU, lambda replicated, each rank holds a contiguous range of the
 * mini-batch's documents.  Documents are independent given lambda (src/lda.cpp:176-214 touches
 * only column i of gamma and ADDS into sstats), so the path's one exchange is the sum of the
 * K x V statistics where the reference has its omp-critical reduction (src/lda.cpp:211-217),
 * plus the V word counts of src/onlinelda.cpp:79-82.  `rccl_comm` is the host program's
 * ncclComm_t (from ncclCommInitRank), passed as an opaque pointer; ncclAllReduce is resolved
 * at run time from the process or librccl.so, and runs on the model's stream. */
/* sstats_dev[K x V] <- sum over ranks */
int trlda_model_allreduce_sstats(trlda_model *model, void *rccl_comm, double *sstats_dev);
/* OnlineLDA::updateParameters (src/onlinelda.cpp:53-111, 177-179) over the ranks of rccl_comm:
 *   shard       this rank's documents [doc_lo, doc_lo + trlda_batch_num_docs(shard)) of a
 *               mini-batch of total_docs
 * gamma0 is drawn for the whole mini-batch from the host stream on every rank (trlda_seed /
 * trlda_rng_set_state keep the ranks' streams equal) and this rank's columns are kept, so an
 * N-rank run reproduces the one-rank trajectory up to the summation order of the all-reduce.
 * Every rank applies the identical M-step: lambda stays replicated without a broadcast. */
int trlda_model_online_update_multi(trlda_model *model, const trlda_batch *shard, void *rccl_comm,
                                    int total_docs, int doc_lo, int num_documents, double eta,
                                    int max_iter_tr, int max_iter_inference, double kappa,
                                    double tau, double rho, int init_gamma, double threshold,
                                    int *update_count, double *rho_out);

/* BatchLDA::updateParameters, lambda path (src/batchlda.cpp:43-61), over the ranks of rccl_comm:
 * max_epochs x { this rank's documents from a fresh random gamma -- its columns of the whole
 * batch's draw, as above; ONE all-reduce of the K x V statistics (src/lda.cpp:211-217 across
 * ranks); lambda = eta + sstats on every rank (src/batchlda.cpp:60) }.  BASELINE config 4: 100 000
 * documents over 8 ranks, 80 MB per all-reduce.  gamma of the shard's documents stays on the
 * device for trlda_model_eb_gamma_stats_multi. */
int trlda_model_batch_update_multi(trlda_model *model, const trlda_batch *shard, void *rccl_comm,
                                   int total_docs, int doc_lo, double eta, int max_epochs,
                                   int max_iter_inference, int update_lambda, double threshold);
/* buf_dev[count] <- sum over ranks (fp64), on the model's stream: the K-vector reduction of
 * src/onlinelda.cpp:128 and any other sum a host composes across ranks */
int trlda_model_allreduce(trlda_model *model, void *rccl_comm, double *buf_dev, size_t count);
/* trlda_model_estep_resident for this rank's documents of a sharded mini-batch (gamma0 = its
 * columns of the whole mini-batch's draw; no exchange, the statistics are not used) */
int trlda_model_estep_resident_shard(trlda_model *model, const trlda_batch *shard, int total_docs,
                                     int doc_lo, int max_iter, double threshold);
/* trlda_model_eb_gamma_stats summed over the ranks' documents: out_host[k] = sum over ALL
 * documents of psi(gamma_dk) - psi(sum_k gamma_dk) (src/onlinelda.cpp:123-128,
 * src/batchlda.cpp:72-74); B = this rank's document count (0 allowed: the rank still takes part
 * in the all-reduce of K doubles).  rccl_comm NULL: this rank's sums only. */
int trlda_model_eb_gamma_stats_multi(trlda_model *model, void *rccl_comm, int B,
                                     const double *gamma_dev, double *out_host /* K */);

/* ---- multi-GPU with FACTOR exchange: an all-gather of 8 (K + n_d) bytes per document --------
 *
 * The same reduction point (src/lda.cpp:211-217), without moving K x V numbers.  lambda is
 * replicated, and sstats[k, w] = expElogbeta[k, w] * sum_{(d, w)} (cnt_dw / phinorm_dw) *
 * expElogtheta[d, k] (src/lda.cpp:207-217): a rank only has to publish, per document, the K
 * numbers expElogtheta[d, :] and one weight per (document, word) entry.  Every rank holds the
 * WHOLE mini-batch (`batch`: word lists, counts -- a few hundred kB) and iterates the documents
 * [doc_cuts[rank], doc_cuts[rank + 1]) of it (`shard`, a batch made of exactly those
 * documents); one ncclAllGather of equal slots follows the document stage, and every rank forms
 * the statistics of the whole mini-batch with the single-GPU kernel -- which adds the entries of
 * a word in document order, the reference's serial order.  Every rank performs the same
 * additions in the same order on the same numbers: the replicas of lambda stay bitwise equal
 * without a broadcast, and they equal the one-GPU result for the whole mini-batch up to the
 * rounding of the document-kernel variant a shard selects (~1e-15; bitwise when the shards and
 * the whole mini-batch select the same variant) -- no dependence on the rank count through an
 * order of summation.  The fused M-step with carried row sums applies unchanged.  Bytes received per rank and E-step: (world - 1) * slot * 8, slot ~
 * max_r(docs_r) * K + max_r(nnz_r): 2.1 MB at K = 100, 8 x 200 documents (the K x V all-reduce
 * moves 9.8 MB per rank); 17 MB at K = 500, 8 x 512 documents (700 MB).  Not the better choice
 * when documents outnumber words (BatchLDA on 8 x 12 500 documents, V = 50 000): compare
 * world * slot with 2 * K * V.
 *
 * `rccl_comm` as above (ncclAllGather, in place, on the model's stream); world = 1 needs none.
 * A host with a transport of its own installs trlda_model_set_allgather instead: the hook is
 * called with this rank's slot (`send` = recv + rank * count), the buffer of world * count
 * doubles and the model's hipStream_t, and must leave every rank's slot in `recv` in stream
 * order; a non-zero return fails the call. */
typedef int (*trlda_allgather_fn)(void *ctx, const void *send_dev, void *recv_dev,
                                  size_t count_f64, void *hip_stream);
int trlda_model_set_allgather(trlda_model *model, trlda_allgather_fn fn, void *ctx);
/* WORD-SHARDED M-STEP (default for world > 1 where a transport for it exists).  After the factor
 * exchange every rank holds every document's factors, so any rank can form any word's statistics:
 * rank r forms statistics + M-step (src/lda.cpp:207-217, src/onlinelda.cpp:99-100,
 * src/batchlda.cpp:60) for ITS contiguous range of the vocabulary only -- the ranges are balanced
 * by the words' entries, the same cut points on every rank -- and the ranks then exchange the
 * lambda columns they wrote, IN PLACE in the replicated table.  Every column is computed once, by
 * its owner, with a word's entries added in document order: the replicas are bitwise equal and
 * equal the one-GPU result.  Per rank and E-step the statistics stage shrinks by the world size
 * (8 x 200 documents, K = 100: 8 us instead of 38 us of kernels), and the second exchange moves
 * the lambda table once (5.6 MB received per rank at K = 100, V = 7000 -- half of what the
 * all-reduce of the statistics moves).  The next E-step's row sums and exp(psi(lambda)) are formed
 * from the exchanged lambda by its own preamble.
 * Transport: `rccl_comm` (one grouped launch of `world` ncclBroadcast calls: ranges of unequal
 * size), or the host's own -- the hook is called with the table, world + 1 offsets in doubles
 * (rank r wrote [offsets[r], offsets[r + 1])), this rank, the world size and the model's
 * hipStream_t, and must leave every range in place in stream order.  Without either (only the
 * equal-slot hook above, or the direct slot exchange) every rank forms the statistics of the
 * whole mini-batch as before.  set_word_sharding(model, 0) does the same by choice. */
typedef int (*trlda_allgatherv_fn)(void *ctx, void *table_dev, const size_t *offsets_f64 /* world + 1 */,
                                   int rank, int world, void *hip_stream);
int trlda_model_set_allgatherv(trlda_model *model, trlda_allgatherv_fn fn, void *ctx);
int trlda_model_set_word_sharding(trlda_model *model, int enabled);
int trlda_model_last_word_sharded(const trlda_model *model);
/* A DIRECT exchange of the slots, behind this switch (the all-gather above stays the default):
 * xGMI is point to point and a slot is a few hundred kB, so every rank writes its slot straight
 * into its peers' gather buffers -- device memory the peers export through hipIpc -- and signals
 * them with a step counter there; no collective launch sits on a step's critical path.
 *   alloc    a region for slots of up to max_slot_f64 doubles (two buffers, alternating per E-step,
 *            + the counters); handle_out receives the 64-byte hipIpcMemHandle_t to give to the peers
 *   connect  handles = world x 64 bytes in rank order (this rank's own is ignored): maps the
 *            peers' regions; the *_dp entry points then use the direct exchange for this world
 *   close    unmaps and frees (also done by trlda_model_destroy)
 * Every rank must make the same sequence of *_dp calls (they do: lambda is replicated).  A peer
 * that never signals makes the next trlda_model_synchronize fail instead of hanging. */
int trlda_model_dp_direct_alloc(trlda_model *model, size_t max_slot_f64, int world, void *handle_out);
int trlda_model_dp_direct_connect(trlda_model *model, int rank, int world, const void *handles);
int trlda_model_dp_direct_close(trlda_model *model);
/* OnlineLDA::updateParameters (src/onlinelda.cpp:53-111, 177-179) over `world` ranks: the
 * arguments of trlda_model_online_update, which it equals for world = 1.  gamma0 is this rank's
 * columns of the whole mini-batch's draw (the stream advances by all of it on every rank). */
int trlda_model_online_update_dp(trlda_model *model, const trlda_batch *batch,
                                 const trlda_batch *shard, void *rccl_comm, int rank, int world,
                                 const int32_t *doc_cuts /* world + 1 */, int num_documents,
                                 double eta, int max_iter_tr, int max_iter_inference, double kappa,
                                 double tau, double rho, int init_gamma, double threshold,
                                 int *update_count, double *rho_out);
/* BatchLDA::updateParameters (src/batchlda.cpp:43-61) with the factor exchange: the arguments of
 * trlda_model_batch_update, which it equals for world = 1.  Pays where the words outnumber the
 * documents' factors (world * slot < 2 K V); BASELINE config 4 is the opposite case
 * (trlda_model_batch_update_multi). */
int trlda_model_batch_update_dp(trlda_model *model, const trlda_batch *batch,
                                const trlda_batch *shard, void *rccl_comm, int rank, int world,
                                const int32_t *doc_cuts /* world + 1 */, double eta, int max_epochs,
                                int max_iter_inference, int update_lambda, double threshold);
/* One E-step (src/lda.cpp:160-220) over `world` ranks: gamma0_dev / gamma_dev hold this rank's
 * K x docs_r columns (gamma0_dev NULL: in place); sstats_dev (K x V, may be NULL with mstep)
 * receives the statistics of the whole mini-batch; iters_dev this rank's iteration counts or
 * NULL.  mstep != 0: the statistics kernel also writes lambda = (1 - rho) lambda' + rho (eta +
 * scale * sstats) for every word (src/onlinelda.cpp:99-100; lambda_prime_dev NULL: lambda'
 * is the current lambda) and leaves the row sums of the new lambda for the next E-step. */
int trlda_model_estep_dp(trlda_model *model, const trlda_batch *batch, const trlda_batch *shard,
                         void *rccl_comm, int rank, int world, const int32_t *doc_cuts,
                         const double *gamma0_dev, double *gamma_dev, double *sstats_dev,
                         int max_iter, double threshold, int32_t *iters_dev, int mstep,
                         const double *lambda_prime_dev, double rho, double eta, double scale);

/* ---- update loop: what stays on the device between its steps ----------------------------
 *
 * Inside one OnlineLDA update lambda' and rho are fixed and a word outside the mini-batch has
 * zero statistics (src/lda.cpp:169), so every M-step of the trust-region loop
 * (src/onlinelda.cpp:99-100) gives it the same value -- the one the initial step of :85-86
 * gives it too.  The update entry points above therefore write those words once per call and
 * run the loop on the batch's active words only, with the statistics (src/lda.cpp:207-217), the
 * M-step and the row sums the next E-step needs (src/lda.cpp:172) in ONE kernel per iteration.
 * The switches below exist for tests and before/after measurements; results do not depend on
 * them beyond summation order. */
/* fused = 0: separate statistics and M-step kernels over all V words (K > 512 always does) */
int trlda_model_set_fused_update(trlda_model *model, int fused);
/* Small tables (K <= 128, K * V < 2^22): while a lambda element is in its registers the M-step
 * kernel also writes exp(psi(.)) of it (src/lda.cpp:173's numerator) and combines the row sums
 * (src/lda.cpp:172) into a few rows, so the next E-step on the same words starts with its
 * document kernel: two launches per trust-region iteration instead of three.  enabled = 0: the
 * next E-step launches its preamble kernel as before (default 1). */
int trlda_model_set_next_preamble(trlda_model *model, int enabled);
/* carry = 0: every E-step adds up the rows of lambda again (src/lda.cpp:172 as written) */
int trlda_model_set_carry_rowsums(trlda_model *model, int carry);
/* keep = 1: the update entry points also leave the sufficient statistics of their last E-step
 * and the complete lambda' on the device (what src/onlinelda.cpp:167-175 reads); costs two
 * K x V writes per call. */
int trlda_model_set_keep_sstats(trlda_model *model, int keep);
/* gamma0 of the update entry points (sampleGamma(K, B, 100) / 100, src/lda.cpp:135) is drawn ON
 * THE DEVICE from the host's libc stream -- the same integers in the same order, hence the same
 * uniforms u, bit for bit -- and the host stream is advanced by the same number of draws.  The
 * device forms -sum_p log|u_p| as -sum over blocks of 25 passes of log(prod_p |u_p|) (one
 * logarithm per 25 draws; the product of 25 values > 2^-31 is a normal double): within 4e-15
 * relative of the host's sum -- which is itself 7e-16 off the exact value, the product form 2e-16
 * (csrc/rng_kernels.h).  host = 1: draw on the host instead, bit for bit the reference's values
 * (K * B * 100 glibc logarithms per call). */
int trlda_model_set_host_gamma_draw(trlda_model *model, int host);
/* The device draw of the NEXT fresh gamma0 of the same shape, made AHEAD of its turn while the current
 * call's kernels run, with the host stream advanced ahead of its turn.  Whatever else touches the
 * generator first -- trlda_seed, a host draw, another model, another shape -- puts the stream back
 * and the draw is repeated in its turn: the ORDER of draws is the reference's in every case
 * (src/lda.cpp:135, src/utils.cpp:224-231).
 *   2 (default)  inside the call's document launch: on small tables (K <= 128, <= 224 document
 *                workgroups) extra workgroups of the launch draw it on the CUs the documents leave
 *                free (csrc/rng_kernels.h, aux_draw_workgroup) -- no launch, no stream of its own;
 *                where the launch cannot carry it the draw is made in its turn;
 *   1            on a stream of the model's own (TRLDA_DRAW_AHEAD=1): gains 13 % at 1600 documents
 *                without trust-region loop, loses where the process has more streams than hardware
 *                queues (bench.py beside torch);
 *   0            every draw in its turn.
 * The values are bitwise the same in all three. */
int trlda_model_set_draw_ahead(trlda_model *model, int enabled);
/* gamma0 draws made inside a document launch so far (tests) */
long long trlda_model_inlaunch_draws(const trlda_model *model);
/* OnlineLDA::updateParameters without trust-region loop (src/onlinelda.cpp:103-109): the decay of the
 * words outside the mini-batch, lambda = (1 - rho) lambda + rho eta, by auxiliary workgroups of the
 * call's document launch (1, the default; small tables) or by the streaming kernel behind it (0).
 * Bitwise the same lambda and row sums either way. */
int trlda_model_set_aux_decay(trlda_model *model, int enabled);
long long trlda_model_inlaunch_decays(const trlda_model *model);   /* (tests) */
/* out_dev[rows x cols] = sampleGamma(rows, cols, passes) / divisor (src/utils.cpp:224-231) on
 * the device, as above (divisor 1 for the bare sum). */
int trlda_model_sample_gamma(trlda_model *model, int rows, int cols, int passes, double divisor,
                             double *out_dev);
/* The columns [col_lo, col_hi) of that matrix only (out_dev: rows x (col_hi - col_lo)); the
 * stream still advances by rows * cols * passes draws.  A data-parallel rank draws its own
 * documents' gamma0 out of the mini-batch's matrix this way, in step with the other ranks. */
int trlda_model_sample_gamma_cols(trlda_model *model, int rows, int cols, int col_lo, int col_hi,
                                  int passes, double divisor, double *out_dev);
/* bytes this model has copied to host memory so far (tests assert that the empirical-Bayes
 * steps move O(K), not O(K V)) */
int64_t trlda_model_d2h_bytes(const trlda_model *model);

/* LDA::updateVariables(documents, parameters) from a fresh random gamma (src/lda.cpp:119-138)
 * with gamma and the statistics left on the device: what src/onlinelda.cpp:118-120 and
 * src/batchlda.cpp:66-68 do before an alpha step when update_lambda is off. */
int trlda_model_estep_resident(trlda_model *model, const trlda_batch *batch, int max_iter,
                               double threshold);

/* out_host[k] = sum_d psi(gamma_dk) - psi(sum_k gamma_dk): the data term of the alpha gradient,
 * src/onlinelda.cpp:123-128, src/batchlda.cpp:72-74, src/cumulativelda.cpp:82-84.
 *   gamma_dev  K x B device array, or NULL: gamma of the model's last update / resident E-step */
int trlda_model_eb_gamma_stats(trlda_model *model, int B, const double *gamma_dev,
                               double *out_host /* K */);

/* *sum_psi_lambda = sum_kw psi(lambda_kw); rowsums_host[k] = sum_w lambda_kw (the host applies
 * psi to those K numbers): the data terms of the eta gradient, src/onlinelda.cpp:152-154,
 * src/batchlda.cpp:152. */
int trlda_model_eb_lambda_stats(trlda_model *model, double *sum_psi_lambda,
                                double *rowsums_host /* K */);

/* ---- empirical Bayes: the K- and scalar-sized host steps (csrc/eb_steps.cpp) --------------- */

/* alpha <- max(alpha - rho H^-1 g, min_alpha): one natural-gradient step, src/onlinelda.cpp:123-142;
 * psi_gamma_diff[k] = sum over the mini-batch's documents of psi(gamma_dk) - psi(sum_k gamma_dk)
 * (trlda_model_eb_gamma_stats), num_docs = the mini-batch's size.  Host memory, no GPU. */
int trlda_eb_online_alpha_step(int K, const double *alpha, const double *psi_gamma_diff,
                               double num_docs, double rho, double min_alpha, double *alpha_out);
/* eta <- max(eta - rho g / h, min_eta): src/onlinelda.cpp:147-162 (sums from
 * trlda_model_eb_lambda_stats) */
double trlda_eb_online_eta_step(double eta, double sum_psi_lambda, const double *rowsums, int K,
                                int V, double rho, double min_eta);
/* Newton steps with a step-halving line search on the lower bound: src/batchlda.cpp:81-141 ==
 * src/cumulativelda.cpp:90-150 (alpha), src/batchlda.cpp:147-205 (eta) */
int trlda_eb_alpha_line_search(int K, const double *alpha, const double *psi_gamma_diff,
                               double num_docs, int max_iter_alpha, double min_alpha,
                               double threshold, double *alpha_out);
double trlda_eb_eta_line_search(double eta, double sum_psi_lambda, const double *rowsums, int K,
                                int V, int max_iter_eta, double min_eta, double threshold);
/* `verbosity` of LDA::Parameters for the two line searches above (per calling thread): above 1 they
 * print their progress to stdout as the reference does (src/batchlda.cpp:78-88,120-123,155-165,
 * 184-187; src/cumulativelda.cpp:87-97,129-132). */
void trlda_eb_set_verbosity(int verbosity);
/* Both online steps after an update, with ONE synchronisation: the device sums over the gamma
 * the update left behind (B_local documents of this rank; summed over the ranks of rccl_comm
 * when that is not NULL) and over lambda, the host steps above, the new alpha back on the
 * device.  alpha_host (K) and *eta are read and updated; B_total = the mini-batch's size. */
int trlda_model_online_eb(trlda_model *model, void *rccl_comm, int B_local, int B_total, double rho,
                          int update_alpha, int update_eta, double min_alpha, double min_eta,
                          double *alpha_host, double *eta);
/* The same in two halves, so that the host can prepare the next mini-batch (parse, convert,
 * upload) while the device still works on this one: _begin enqueues the sums and their way back
 * to pinned host memory and returns; _finish waits for them, takes the steps and puts the new
 * alpha on the device.  Between the two the model runs no E-step (TRLDA_ERR_ARG): the caller
 * finishes before its next call -- trlda.models.OnlineLDA does, at the start of the next
 * update_parameters / do_e_step / lower_bound and in the alpha / eta getters.  _pending: 1 between
 * the halves. */
int trlda_model_online_eb_begin(trlda_model *model, void *rccl_comm, int B_local, int B_total,
                                int update_alpha, int update_eta);
int trlda_model_online_eb_finish(trlda_model *model, double rho, double min_alpha, double min_eta,
                                 double *alpha_host, double *eta);
int trlda_model_online_eb_pending(const trlda_model *model);
/* test hook: psi and psi' as eb_steps.cpp evaluates them */
void trlda_debug_host_psi(int n, const double *x, double *psi_out, double *psi1_out);

/* Adaptive learning rate, src/onlinelda.cpp:167-172, after an update made with keep_sstats on:
 * lambdaUpdate = (eta + scale * sstats) - lambda'; the model's running average
 * mAdaGradient = (1 - 1/tau) mAdaGradient + 1/tau lambdaUpdate (K x V, device, zero at first);
 * returns |lambdaUpdate|^2 and |mAdaGradient|^2.  eta: the value the update used. */
int trlda_model_adaptive_stats(trlda_model *model, double eta, double scale, double tau,
                               double *sq_norm_update, double *sq_norm_gradient);

/* The same with the statistics and lambda' given as device arrays (K x V each): for a host that
 * composes the data-parallel update itself (E-step -> all-reduce -> blend) and holds both. */
int trlda_model_adaptive_stats_dev(trlda_model *model, const double *sstats_dev,
                                   const double *lambda_prime_dev, double eta, double scale,
                                   double tau, double *sq_norm_update, double *sq_norm_gradient);

/* ---- test hook ----------------------------------------------------------- */

/* The device digamma (TRLDA::digamma, src/digamma.cpp:116-178, as compiled for gfx950)
 * evaluated at n host points: psi[i] = psi(x[i]); epsi[i] = exp(psi(x[i])) in the log-free
 * form the hot path uses (lda.cpp:173-174, :197 only ever need exp(psi)); epsi_lean[i] = the
 * call-free form for positive arguments that the M-step kernels use when they leave the next
 * E-step's exp(psi(lambda)) behind (bitwise the same except at the integers 1..10, where the
 * reference's exact harmonic branch and the regular form differ by a few ulp; for x <= 0 the
 * general form); eminus[i] = exp(psi(x[i]) - c)
 * (lda.cpp:173).  Lets the parity tests check the special functions against the reference's
 * table directly. */
int trlda_debug_digamma(int device, int n, double c, const double *x, double *psi, double *epsi,
                        double *epsi_lean, double *eminus);
/* test hook: the transposing wave reductions of csrc/estep_wide.h on a 64 x 16 table
 * (row = lane); out16 / out4 / out2 [64] = what each lane receives from the 16-, 4- and
 * 2-value folds of its row's leading values */
int trlda_debug_fold16(int device, const double *in, double *out16, double *out4, double *out2);
/* diagnostics: copy out one of the model's intermediate buffers of its last E-step (after
 * synchronising its stream).  which = 0: exp(psi(lambda)) / exp E[log beta] as the kernels read it
 * (K x V; only the batch's words are filled), 1: the documents' exp E[log theta] rows, 2: cnt /
 * phinorm per entry in word order, 3: the sstats buffer of the host entry points (K x V).
 * tests/fuzz_estep.py --passes uses it to say WHICH input of the statistics went wrong. */
int trlda_debug_peek(trlda_model *model, int which, double *host_out, size_t count);
/* test hook: the normalised exp E[log beta] table the model's last Gibbs call sampled from
 * (K x V; only that batch's words are filled) -- the tests' restatement of the sampler
 * (tests/gibbs_host.py) reads the same numbers the kernel did.  The table shares its memory with
 * trlda_model_sample's: after a sample call this fails until the next Gibbs call. */
int trlda_debug_gibbs_table(trlda_model *model, double *host_out);
/* test hook: the beta prefix table the model's last trlda_model_sample call read (K x V,
 * TOPIC-MAJOR: element (k, w) at [w + V*k]; csrc/sample_kernels.h).  Fails after a Gibbs call. */
int trlda_debug_sample_table(trlda_model *model, double *host_out);
/* test hook: trlda_sample_dirichlet_device's draws under `key` stopped before the divide: w_out
 * (m x n, host) gets W = exp(lg - column max), sums_out (n, host) the column sums S in the order
 * csrc/dirichlet_kernels.h states (tests/dirichlet_host.py restates it from these W). m, n > 0. */
int trlda_debug_dirichlet_sums(int m, int n, double alpha, uint64_t key, double *w_out, double *sums_out,
                               int device);
/* diagnostics: the s_memrealtime stamps of the model's last merged launch, 3 x 1024 values
 * (TRLDA_MERGED_STAMPS=1; tools/merged_stamps.py) */
int trlda_debug_merged_stamps(trlda_model *model, unsigned long long *host_out);
/* test hook: the device allocations the library's own buffers -- those of models, coherence
 * accumulators, document indexes and temporaries; not batches, not trlda_dev_alloc's -- hold now
 * (*live) and have made so far (*total) in this process.  With every handle destroyed, *live is 0
 * (tests/test_gpu_buffers.py). */
int trlda_debug_device_buffers(long long *live, long long *total);

/* ---- measurement --------------------------------------------------------- */

/* Average duration in microseconds (HIP events on the model's stream) of the
 * kernels launched by the most recent trlda_model_estep when timing is on:
 * which = 0 row sums (or the fused preamble, then 1 is empty), 1 exp E[log beta],
 * 2 per-document fixed point, 3 sufficient statistics, 4 nothing: two event records back to
 * back, i.e. the part of every other figure that is the events' own cost.  Timing adds
 * event records to the stream. */
int trlda_model_set_timing(trlda_model *model, int enabled);
int trlda_model_get_timing(trlda_model *model, int which, double *usec_sum, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* TRLDA_HIP_H */
