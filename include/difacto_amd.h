/*
 * difacto_amd.h — the C-ABI of libdifacto_amd.so, the MI355X (gfx950) implementation of
 * DiFacto's data-parallel hot path.
 *
 * Plain pointers and sizes only (no C++ or torch types).  Every function returns a status
 * (DFX_OK == 0); on failure dfx_last_error() holds the message.  The C++ adapters under
 * difacto_amd/host map a non-zero status to LOG(FATAL), which is the reference's own error
 * convention (CHECK / LOG(FATAL) abort, include/difacto/base.h + dmlc logging).
 *
 * POINTERS: every array argument is a DEVICE pointer (hipMalloc / dfx_malloc / a torch
 * tensor's data_ptr()) on the context's device; scalar outputs (int64_t*, double*) are host
 * pointers.  Work is queued on the context's stream (dfx_ctx_set_stream); functions whose
 * result is a host scalar synchronise that stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   Localizer::Compact            src/data/localizer.h:41-51, localizer.cc:11-107
 *   FMLoss::Predict / CalcGrad    src/loss/fm_loss.h:56-119, 136-203
 *   LogitLoss::Predict / CalcGrad src/loss/logit_loss.h:41-57, 71-103   (== FM with V_dim 0)
 *   Loss::Evaluate                include/difacto/loss.h:57-66
 *   BinClassMetric::AUC           src/loss/bin_class_metric.h:35-57
 *   SGDLearner::GetPos            src/sgd/sgd_learner.cc:151-165
 *   Store::Push / Pull            include/difacto/store.h:44-75 (StoreLocal store_local.h:24-45,
 *                                 KVStoreDist kvstore_dist.h:90-107)
 *   SGDUpdater::Get / Update      src/sgd/sgd_updater.cc:34-152 (FTRL w, AdaGrad V, InitV)
 *   SGDUpdater::Save/Load/Dump    src/sgd/sgd_updater.h:84-139
 *   SGDUpdater::Evaluate          src/sgd/sgd_updater.cc:12-30
 *   SGDLearner::IterateData body  src/sgd/sgd_learner.cc:201-317 (fused: dfx_train_step)
 */
#ifndef DIFACTO_AMD_H_
#define DIFACTO_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_OK 0
#define DFX_ERR_ARG 1      /* bad argument (shape, null pointer, unsupported V_dim) */
#define DFX_ERR_HIP 2      /* a HIP runtime call failed */
#define DFX_ERR_CAPACITY 3 /* hash table or V pool full (see dfx_store_reserve) */
#define DFX_ERR_CHECK 4    /* a reference CHECK failed (e.g. lens[i] != V_dim+1) */
#define DFX_ERR_IO 5       /* model file could not be read / written */

/* value types, include/difacto/store.h:33-35 */
#define DFX_FEA_COUNT 1
#define DFX_WEIGHT 2
#define DFX_GRADIENT 3

/* job types, src/sgd/sgd_utils.h:14-20 */
#define DFX_JOB_TRAINING 3
#define DFX_JOB_VALIDATION 4
#define DFX_JOB_PREDICTION 5

typedef struct dfx_ctx dfx_ctx;

/* dmlc::RowBlock<feaid_t> as produced by BatchReader (device pointers). */
typedef struct dfx_batch {
  int64_t size;           /* B rows */
  int64_t nnz;            /* == offset[B] */
  const uint64_t* offset; /* B+1 (size_t), offset[0] == 0 */
  const uint64_t* index;  /* nnz raw feature ids */
  const float* value;     /* nnz, or NULL for binary data (batch_reader.cc:71-73) */
  const float* label;     /* B */
  const float* weight;    /* B row weights, or NULL */
} dfx_batch;

/* sgd::Progress (src/sgd/sgd_utils.h:52-93), accumulated in double. auc is AUC*rows. */
typedef struct dfx_progress {
  double nrows;
  double loss;
  double auc;
  double penalty;
  double nnz_w;
} dfx_progress;

/* ---- context -------------------------------------------------------------------------
 * kwargs: the reference .conf keys, "k=v" separated by ',', ';', ' ' or newlines:
 *   loss (fm|logit), V_dim, lr, lr_beta, l1, l2, V_lr, V_lr_beta, V_l2, V_init_scale,
 *   V_threshold, l1_shrk, seed          (sgd_param.h:79-123, fm_loss.h:19-27)
 * plus device-store sizing: max_keys (hash table keys, default 1<<22; the table grows by
 * itself at sync points, autogrow=0 turns that off), max_vrows (V pool rows of the split
 * layout, default max_keys); the store's slot layout: slot_layout=auto|split|fat (auto: a key's
 * entry and V share one 64/128-byte slot when 4 <= V_dim <= 24 and V_dim % 4 == 0); the
 * sharded store's push_agg=sum|ranks and hash=ordered|mixed; and execution choices that do
 * not change results (A/B switches, measured in DESIGN.md): fwd_probe, xvp_row, bwd_lds,
 * sort_pack, sort_items, sort_lookback, auc_sort=radix|merge|bucket|wbucket, fat_fwd, fat_bwd,
 * initv_onepass, fat_nb, fwd_ids, fwd_pf, lr_lanes, loc_bucket, lb_wave, lb_keyfirst,
 * lb_gather=0|1|2, lb_tiles, lb_hnt=256|512|1024, lb_xcd, auc_db=0|1|2, lane_after_fwd,
 * lane_prio.  Unknown keys are ignored (InitAllowUnknown). */
const char* dfx_last_error(void);
int dfx_ctx_create(int device, const char* kwargs, dfx_ctx** out);
int dfx_ctx_destroy(dfx_ctx* ctx);
/* A new context queues work on its own non-blocking stream.  set_stream switches to the given
 * hipStream_t (NULL = the null stream, torch's default); use_own_stream switches back. */
int dfx_ctx_set_stream(dfx_ctx* ctx, void* hip_stream);
int dfx_ctx_use_own_stream(dfx_ctx* ctx);
/* the context's streams (hipStream_t): which = 0 the Localizer lane, 1 the AUC lane, 2 the
 * split partition's stream, 3 the context stream itself */
int dfx_ctx_lane_stream(dfx_ctx* ctx, int which, void** out);
/* run the Localizer lane (which = 0) or the split partition (which = 2) on the caller's stream
 * (it must outlive the context's use of it; NULL: back to the library's own), e.g. a stream of
 * the caller's framework, whose allocator then tracks buffers used on it */
int dfx_ctx_set_lane_stream(dfx_ctx* ctx, int which, void* hip_stream);
/* The stream on which dfx_train_step's batches are produced (a loader / copy stream; NULL =
 * the context stream).  A batch's Localizer waits only for that stream, so it can run while
 * the context stream is still on the previous batch's forward / backward.  The caller keeps a
 * batch's buffers alive until the context stream has passed the dfx_train_step that took it. */
int dfx_ctx_set_input_stream(dfx_ctx* ctx, void* hip_stream);
int dfx_ctx_vdim(dfx_ctx* ctx);
int dfx_sync(dfx_ctx* ctx); /* waits for the stream and reports deferred device errors */
/* waits for the input stream (the context stream when none is set): a batch that was produced
 * and copied there (dfx_batchcache_append) but never stepped is then done with its producer's
 * buffers, which the producer's `consumed` marks would otherwise tie to a step */
int dfx_sync_input(dfx_ctx* ctx);
int dfx_malloc(dfx_ctx* ctx, void** ptr, size_t bytes);
int dfx_free(dfx_ctx* ctx, void* ptr);
/* kind: 0 host->device, 1 device->host, 2 device->device; async on the stream.  A pageable
 * host source may be reused when the call returns (HIP stages it during the call, measured
 * behind a busy stream by tools/pageable_probe.hip); a pinned one only after the copy ran.
 * Device->host returns once the data are on the host. */
int dfx_memcpy(dfx_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
/* pre-size the fused-path workspace so dfx_train_step allocates nothing */
int dfx_reserve(dfx_ctx* ctx, int64_t max_rows, int64_t max_nnz);

/* ---- batch feeder (SGDLearner::IterateData's producer loop, sgd_learner.cc:289-314) -----
 * Host RowBlocks to device batches through pinned staging and a loader stream that becomes
 * the context's input stream; two slots, so the upload of batch t+1 overlaps the step on t.
 *   dfx_feeder_slot     the next slot's pinned host arrays (waits until the step that used
 *                       the slot two batches ago has passed the device); fill them
 *   dfx_feeder_submit   enqueue their upload; *out receives the device batch
 *   dfx_feeder_consumed after dfx_train_step(*out): marks the slot in use until then */
typedef struct dfx_feeder dfx_feeder;
typedef struct dfx_host_batch {
  uint64_t* offset; /* max_rows + 1 */
  uint64_t* index;  /* max_nnz */
  float* value;     /* max_nnz */
  float* label;     /* max_rows */
  float* weight;    /* max_rows */
  int64_t max_rows;
  int64_t max_nnz;
} dfx_host_batch;
int dfx_feeder_create(dfx_ctx* ctx, int64_t max_rows, int64_t max_nnz, dfx_feeder** out);
int dfx_feeder_destroy(dfx_feeder* f);
int dfx_feeder_slot(dfx_feeder* f, dfx_host_batch* hb);
int dfx_feeder_submit(dfx_feeder* f, int64_t B, int64_t nnz, int has_value, int has_weight,
                      dfx_batch* out);
int dfx_feeder_consumed(dfx_feeder* f);
/* nslots (2..8) staging slots; dfx_feeder_consumed_back(f, k) marks the slot of the batch
 * submitted k submits ago — a pipelined consumer (the split driver runs step t when step t+1
 * is submitted) marks batch t after the call that queued its last reader */
int dfx_feeder_create_slots(dfx_ctx* ctx, int64_t max_rows, int64_t max_nnz, int nslots,
                            dfx_feeder** out);
int dfx_feeder_consumed_back(dfx_feeder* f, int back);

/* ---- Criteo text on the device (difacto_amd/csrc/textparse.hip) --------------------------
 * dfx_parse_criteo replaces CriteoParser::ParseBlock (src/reader/criteo_parser.h:40-92) for a
 * chunk of whole lines text_dev[0, nbytes) in device memory: offset[rows + 1] (offset[0] == 0),
 * index[nnz] = (CityHash64(cell) << 12) | column for every non-empty cell of the first 39
 * feature columns, label[rows]; is_train == 0 is criteo_test (no label column, labels 0).
 * The result equals the host reader's ParseCriteo (difacto_amd/host/reader.cc) byte for byte,
 * or the chunk is flagged: stat_dev[4] (device) = {rows, nnz, needs_host, overflow}.
 * needs_host == 1: the outputs are undefined and the host parses the chunk.  Only these forms
 * may raise it: a label cell that is not [+-]?[0-9]{1,9} filling the cell (an empty one too),
 * a '\r' byte anywhere, an empty line, a last byte that is not '\n'.
 * overflow == 1: the chunk needs more than max_rows rows or max_nnz ids; rows / nnz then hold
 * the needed counts (with more than 2 * max_rows + 1 lines: the upper bounds lines and
 * 39 * lines) and nothing was written.  No byte outside the text is read, nothing past the
 * capacities is written.  nbytes >= 2^31 is DFX_ERR_ARG (positions are 32-bit).
 * dfx_gather_rows replaces the row copies of BatchReader (src/reader/batch_reader.cc:29-78;
 * the host reader's GatherRows): rows rows_dev[0..n) of a source CSR (rows_dev NULL: rows
 * [begin, begin + n)) appended to a destination CSR at row r0, offsets rebased onto
 * dst_offset[r0] (0 when r0 == 0), labels copied; the caller sizes the destination.
 * Both are asynchronous on the context's input stream (dfx_ctx_set_input_stream; none: the
 * context stream), beside the step like the feeder's copies.  dfx_parse_criteo_wait joins that
 * stream, copies the four counts to stat (host) and returns DFX_ERR_CAPACITY on overflow. */
int dfx_parse_criteo(dfx_ctx* ctx, const char* text_dev, int64_t nbytes, int is_train,
                     int64_t max_rows, int64_t max_nnz, uint64_t* offset, uint64_t* index,
                     float* label, int64_t* stat_dev);
int dfx_parse_criteo_wait(dfx_ctx* ctx, const int64_t* stat_dev, int64_t* stat);
int dfx_gather_rows(dfx_ctx* ctx, const uint64_t* src_offset, const uint64_t* src_index,
                    const float* src_label, const uint32_t* rows_dev, int64_t begin, int64_t n,
                    uint64_t* dst_offset, uint64_t* dst_index, float* dst_label, int64_t r0);

/* ---- libsvm text on the device (difacto_amd/csrc/libsvmparse.hip) ------------------------
 * dfx_parse_libsvm replaces the libsvm branch of TextReader::ParseChunk (the host reader's
 * ParseLibSVM, difacto_amd/host/reader.cc; libsvm is the reference's default data_format,
 * sgd_param.h:57) for a chunk of whole lines text_dev[0, nbytes) in device memory:
 * offset[rows + 1] (offset[0] == 0), index[nnz], value[nnz] (always written: 1.0f for a bare
 * id, as ParseLibSVM does), label[rows], and rowflag[rows] (bytes): 1 iff the row holds a value
 * whose bits are not 1.0f's, so a batch has values iff one of its rows is flagged
 * (BatchReader::Next's all-ones test, batch_reader.cc:71-73, with no read-back).
 * Numbers are converted by csrc/strtof.h: glibc strtof's correctly rounded result bit for bit
 * inside its fast grammar  [+-]? (digits ('.' digits?)? | '.' digits) ([eE] [+-]? digits{1,3})?
 * with at most 19 digits after the leading zeros and |exponent - fraction digits| <= 27.
 * Parsed on the device: lines  label (blank+ feature)* blank* '\n',  blank = ' ' | '\t',
 * blanks before the label allowed, feature = digits | digits ':' number, label and number in
 * the fast grammar; an id is any run of digits and saturates to 2^64 - 1 as strtoull does;
 * rows with no feature.  The result equals ParseLibSVM's byte for byte, or the chunk is
 * flagged: stat_dev[4] (device) = {rows, nnz, needs_host, overflow}, as dfx_parse_criteo's.
 * needs_host == 1: the outputs are undefined and the host parses the chunk.  Only these forms
 * may raise it: a label or value outside the fast grammar; a feature that is not digits or
 * digits ':' number; a token longer than 64 bytes; a '\r' byte anywhere; an empty or
 * blank-only line; a last byte that is not '\n'.
 * overflow == 1: the chunk needs more than max_rows rows or max_nnz features; rows / nnz hold
 * the needed counts and nothing was written.  No byte outside the text is read, nothing past
 * the capacities is written.  nbytes >= 2^31 is DFX_ERR_ARG.  Asynchronous on the context's
 * input stream; dfx_parse_criteo_wait serves as the wait.
 * dfx_gather_rows_valued is dfx_gather_rows with the values and the row flags gathered
 * alongside.  src_value NULL: the source is binary and reads as ones (GatherRows's rule);
 * dst_value NULL: values are dropped; src_rowflag NULL: flags 0; dst_rowflag NULL: none kept. */
int dfx_parse_libsvm(dfx_ctx* ctx, const char* text_dev, int64_t nbytes, int64_t max_rows,
                     int64_t max_nnz, uint64_t* offset, uint64_t* index, float* value,
                     float* label, uint8_t* rowflag, int64_t* stat_dev);
int dfx_gather_rows_valued(dfx_ctx* ctx, const uint64_t* src_offset, const uint64_t* src_index,
                           const float* src_value, const float* src_label,
                           const uint8_t* src_rowflag, const uint32_t* rows_dev, int64_t begin,
                           int64_t n, uint64_t* dst_offset, uint64_t* dst_index, float* dst_value,
                           float* dst_label, uint8_t* dst_rowflag, int64_t r0);

/* ---- adfea text on the device (difacto_amd/csrc/adfeaparse.hip) --------------------------
 * dfx_parse_adfea replaces the adfea branch of TextReader::ParseChunk (the host reader's
 * ParseAdfea, difacto_amd/host/reader.cc; the reference's CTR format,
 * src/reader/adfea_parser.h:34-84) for a chunk of whole lines text_dev[0, nbytes) in device
 * memory: offset[rows + 1] (offset[0] == 0), index[nnz], label[rows]; the rows are binary.
 * Parsed on the device: lines
 *   blank* digits blank+ digits blank+ digits (blank+ digits ':' digits)* blank* '\n'
 * with blank = ' ' | '\t'.  A line's tokens 0 and 1 (lineid, count) are checked and dropped;
 * token 2 is the label, 1.0f iff its first byte is '1' (the reference's rule: "10" is 1, "01"
 * is 0); every later token idx:gid is a feature (idx << 12) | (gid & 4095), idx and gid any run
 * of digits, saturating to 2^64 - 1 as strtoull does, the shift wrapping mod 2^64 as the
 * host's.  rows = newlines, nnz = tokens - 3 * rows.  Inside this domain ParseAdfea's result
 * does not depend on where ParseChunk cuts the chunk for its threads (it cuts at newlines and
 * the parser's token counter is back at 0 after every such line).  The result equals
 * ParseAdfea's byte for byte, or the chunk is flagged: stat_dev[4] (device) = {rows, nnz,
 * needs_host, overflow}, as dfx_parse_criteo's.
 * needs_host == 1: the outputs are undefined and the host parses the chunk.  Only these forms
 * may raise it: an empty or blank-only line; a line with fewer than three tokens; one of a
 * line's first three tokens that is not digits (an "idx:gid" there is the host's row continued
 * on the next line, which the device leaves to it); a later token that is not digits ':'
 * digits; a token longer than 64 bytes; a '\r' byte anywhere; a last byte that is not '\n'.
 * overflow == 1: the chunk needs more than max_rows rows or max_nnz features; rows / nnz hold
 * the needed counts and nothing was written.  No byte outside the text is read, nothing past
 * the capacities is written.  nbytes >= 2^31 is DFX_ERR_ARG.  Asynchronous on the context's
 * input stream; dfx_parse_criteo_wait serves as the wait. */
int dfx_parse_adfea(dfx_ctx* ctx, const char* text_dev, int64_t nbytes, int64_t max_rows,
                    int64_t max_nnz, uint64_t* offset, uint64_t* index, float* label,
                    int64_t* stat_dev);

/* The text feed (difacto_amd/csrc/textfeed.hip): raw text to device batches
 * (src/reader/reader.h:18-55 + batch_reader.cc with the parsing and the row copies on the
 * device).  nslots pinned text slots, a loader stream that becomes the context's input stream,
 * one parsed chunk (device CSR + pinned copies of its offsets and labels) per slot, a shuffle
 * buffer of shuf_rows rows and a ring of nring device batches of batch_rows rows.  The format
 * (DFX_TEXT_CRITEO, DFX_TEXT_LIBSVM, DFX_TEXT_ADFEA) is fixed at creation and every call below
 * takes its behaviour from the feed.  A Criteo feed holds 39 ids a row at most: rows size
 * everything.
 *   dfx_textfeed_text      the slot's pinned text buffer, at least `bytes` long; fill it
 *   dfx_textfeed_submit    upload + the format's parser + the copies back, asynchronous
 *   dfx_textfeed_wait      join: stat[4] as dfx_parse_criteo_wait, the pinned offsets / labels
 *   dfx_textfeed_upload    a chunk the host parsed (needs_host) into the slot's arrays
 *   dfx_textfeed_batch_begin / _gather / _batch_end   form the next ring batch: gathers from
 *                          a slot's chunk (src >= 0) or the shuffle buffer (src == -1) into
 *                          the batch (to_batch) or the shuffle buffer, rows a HOST list or
 *                          NULL for the range [begin, begin + n), appended at row r0
 *   dfx_textfeed_consumed  after dfx_train_step(*out): the ring entry is in use until then
 *   dfx_textfeed_slot_batch / _slot_consumed   a slot's whole chunk as one batch (validation
 *                          reads 256 MB chunks as batches, sgd_learner.cc:281-286)
 * A libsvm feed is valued: every CSR also holds values and row flags (dfx_parse_libsvm) and has
 * an nnz capacity of its own.  A slot's is the submit's max_nnz (the chunk's blanks bound its
 * features; a Criteo feed ignores it, and a libsvm feed is_train); the shuffle buffer's and a
 * ring entry's grow on demand (x 1.25) keeping their contents, by the nnz a gather says it
 * appends (the caller knows the row lengths).  _wait and _upload also hand out the slot's pinned
 * row flags (NULL on a Criteo feed); _upload computes them from the values, and may move all
 * three pinned arrays.  _batch_end / _slot_batch with valued == 0 hand out value == NULL: the
 * caller found no flagged row in the batch (batch_reader.cc:71-73).  On a Criteo feed a value
 * array, a gather's nnz != 0 and valued != 0 are DFX_ERR_ARG, as is an _upload with features
 * and no value array on a libsvm feed; a rejected call queues nothing.
 * A DFX_TEXT_ADFEA feed (dfx_parse_adfea) is sized by nnz as a libsvm feed is (the submit's
 * max_nnz: the ':' bytes of a chunk inside the parser's domain bound its features, and a chunk
 * that needs more is outside it; the growth; the nnz a gather says it appends) and binary as a
 * Criteo feed is: no value arrays, no row flags, the pinned row flag pointers NULL, _upload
 * takes value == NULL; a value array and valued != 0 are DFX_ERR_ARG. */
typedef struct dfx_textfeed dfx_textfeed;
enum { DFX_TEXT_CRITEO = 0, DFX_TEXT_LIBSVM = 1, DFX_TEXT_ADFEA = 2 };
int dfx_textfeed_create(dfx_ctx* ctx, int nslots, int nring, int64_t batch_rows,
                        int64_t shuf_rows, int format, dfx_textfeed** out);
int dfx_textfeed_destroy(dfx_textfeed* f);
int dfx_textfeed_text(dfx_textfeed* f, int slot, int64_t bytes, char** pinned);
int dfx_textfeed_submit(dfx_textfeed* f, int slot, int64_t nbytes, int is_train,
                        int64_t max_rows, int64_t max_nnz);
int dfx_textfeed_wait(dfx_textfeed* f, int slot, int64_t* stat, const uint64_t** offset_host,
                      const float** label_host, const uint8_t** rowflag_host);
int dfx_textfeed_upload(dfx_textfeed* f, int slot, int64_t rows, int64_t nnz,
                        const uint64_t* offset, const uint64_t* index, const float* value,
                        const float* label, const uint8_t** rowflag_host);
int dfx_textfeed_batch_begin(dfx_textfeed* f);
int dfx_textfeed_gather(dfx_textfeed* f, int src, int to_batch, const uint32_t* rows,
                        int64_t begin, int64_t n, int64_t r0, int64_t nnz);
int dfx_textfeed_batch_end(dfx_textfeed* f, int64_t rows, int64_t nnz, int valued,
                           dfx_batch* out);
int dfx_textfeed_consumed(dfx_textfeed* f);
/* Late marking, for callers whose step is not queued when their call returns (the sharded
 * stores run step t at submit t + 1 or at a flush): marks the ring entry begun `back`
 * dfx_textfeed_batch_begin calls ago (0: the current one; back < nring), after the call that
 * queued its last reader and before _batch_begin comes round to it.  A slot batch is marked late
 * with dfx_textfeed_slot_consumed, which names its slot; the slot must not be filled or
 * submitted again before.  dfx_textfeed_counts: the feed's slot and ring counts and the ring
 * entry last begun (-1: none); any of the three may be NULL. */
int dfx_textfeed_consumed_back(dfx_textfeed* f, int back);
int dfx_textfeed_counts(dfx_textfeed* f, int* nslots, int* nring, int* cur);
int dfx_textfeed_slot_batch(dfx_textfeed* f, int slot, int valued, dfx_batch* out);
int dfx_textfeed_slot_consumed(dfx_textfeed* f, int slot);

/* ---- device batch cache (difacto_amd/csrc/batchcache.hip) --------------------------------
 * Formed batches kept in device memory, so that every epoch after the first replays them with
 * no reader, no upload and no parse: a reader lives for one part of one epoch and seeds its
 * shuffle and down-sampling afresh (batch_reader.cc:12-27), so a part yields the same batches
 * in every epoch.  A list is an ordered sequence of batches under a caller-chosen id >= 0 (the
 * driver: one per job kind and part).
 *   dfx_batchcache_begin   opens a list for recording (one at a time; an id only once)
 *   dfx_batchcache_append  adds a copy of *src: byte for byte its offset[B+1], index[nnz] and
 *                          label[B], and value[nnz] / weight[B] when it has them (NULL stays
 *                          NULL); *kept = 1.  Device-to-device copies, asynchronous on the
 *                          context's input stream (dfx_ctx_set_input_stream; none: the context
 *                          stream): behind the producer of *src, before that stream reuses its
 *                          buffers, no host wait
 *   dfx_batchcache_seal    closes the open list; *n_batches its length, -1 if it was dropped
 *   dfx_batchcache_count   *n_batches of a sealed list, -1 dropped, -2 never begun
 *   dfx_batchcache_get     batch i of a sealed list, its pointers into the cache: valid until
 *                          destroy, ready by the input stream's order, and good for
 *                          dfx_train_step, dfx_dist_localize, ... any number of times
 *   dfx_batchcache_stats   out[4] = {lists sealed, lists dropped, batches held, bytes allocated}
 * Memory: device blocks of block_bytes (0: 64 MiB), each owned by one list and never moved; an
 * array larger than a block has an allocation of its own; every array starts on a 256-byte
 * boundary, as allocations do (the step's kernels read them with vector loads).  budget_bytes
 * bounds the sum of the allocations, and a hipMalloc out of memory counts as over budget.  An
 * append that does not fit drops the open list: *kept = 0 with DFX_OK (so do later appends),
 * its blocks are freed after joining the stream that copies into them, get on it is
 * DFX_ERR_ARG; sealed lists are untouched and a later list may use the freed budget.  Training
 * never fails because the cache could not grow.  destroy joins the context (dfx_sync) first; with
 * a live reshuffler (dfx_reshuffle_create) it is DFX_ERR_ARG and the cache stays.
 * DFX_ERR_ARG: append / seal with no open list, begin while one is open or of an id already
 * sealed or dropped, get of an open list or with i out of range, negative sizes, a batch with
 * rows but no offset or label. */
typedef struct dfx_batchcache dfx_batchcache;
int dfx_batchcache_create(dfx_ctx* ctx, int64_t budget_bytes, int64_t block_bytes,
                          dfx_batchcache** out);
int dfx_batchcache_destroy(dfx_batchcache* bc);
int dfx_batchcache_begin(dfx_batchcache* bc, int64_t list);
int dfx_batchcache_append(dfx_batchcache* bc, const dfx_batch* src, int* kept);
int dfx_batchcache_seal(dfx_batchcache* bc, int64_t* n_batches);
int dfx_batchcache_count(dfx_batchcache* bc, int64_t list, int64_t* n_batches);
int dfx_batchcache_get(dfx_batchcache* bc, int64_t list, int64_t i, dfx_batch* out);
int dfx_batchcache_stats(dfx_batchcache* bc, int64_t* out); /* out[4] */

/* ---- the Localizer's outputs kept with a cached batch (batchcache.hip, step.hip) ----------
 * A batch's Localizer output depends on the batch and max_index alone, not on the model, so a
 * replayed epoch's Localizer lane recomputes bit for bit what the recording epoch's computed.
 * Opt-in: the recording epoch keeps, next to a cached batch, what the main stream of
 * dfx_train_step reads of its lane's work (dfx_localize_occ's terms): uniq[U],
 * segstart[U + 1], occ_row[nnz]; for a valued batch occ_x[nnz], or (lb_gather=2) rowof[2 nnz]
 * with occ_row holding input positions — whichever form the lane produced, replayed as that
 * form; when the chunk plan holds chunks, choff[U] and chunk_seg[n_chunks]; and the totals
 * record, four device words {U, n_chunks, the plan's gate, 0}: every word of the lane's device
 * state that the probe, the count push, the chunk kernels, the fused backward, InitV or the
 * finalize read.  Not kept: the keys' table slots, the InitV flags and whatever else depends on
 * the model — a table that grows between record and replay does not matter.
 * Memory: exact sizes by what the lane produced (not the nnz bound), from the open list's
 * blocks, each array on a 256-byte boundary, inside the same budget as the batches.  Where
 * U ~ nnz (uniform keys, the C3 shape) that is ~16 B/nnz (8 uniq + 4 segstart + 4 occ_row)
 * beside the batch's 8 B/nnz, about three times the cache without the outputs; on skewed data
 * U << nnz and it is nearer 4 B/nnz.
 *   dfx_batchcache_append_loc  after the dfx_train_step (on the cache's context) that consumed
 *                          the batch last appended, from that batch's pointers or its
 *                          source's: keeps that step's Localizer outputs with that batch;
 *                          *kept = 1.  The lane's sizes {U, n_chunks, gate} reach a pinned host
 *                          record by one small kernel queued on the lane's stream; the host
 *                          waits for that lane alone, never for the context stream, then
 *                          queues one kernel (k_loc_pack: a by-value table of {source,
 *                          destination, bytes}, 16-byte vector moves) on the lane's stream,
 *                          behind the lane and before that stream reuses the parity's buffers.
 *                          Outputs that do not fit the budget: *kept = 0 with DFX_OK, the batch
 *                          stays cached without them and the list is NOT dropped.
 *                          DFX_ERR_ARG: no open list, nothing appended since begin, a second
 *                          call for one batch or one step, the context's last step ran no
 *                          Localizer (none yet, or a replayed one) or was of another B or nnz
 *   dfx_batchcache_get_loc     batch i of a sealed list: *out, pointers into the cache as get's;
 *                          out->uniq == NULL (DFX_OK) for a batch without outputs.  Callers
 *                          pass the struct on and read only uniq (tests: its arrays)
 *   dfx_train_step_loc         dfx_train_step whose lane does not run the Localizer and the
 *                          chunk plan: on the same lane stream, behind the same waits (the
 *                          input, the parity's last user) and before the same join and event
 *                          record, one one-block kernel (k_loc_install) writes the totals record
 *                          into the parity's device state, and the step's kernels read the
 *                          arrays in the cache.  Same results, bit for bit, for every job type
 *                          and with push_cnt (the counts are the segment lengths).  loc NULL or
 *                          loc->uniq NULL: dfx_train_step.  DFX_ERR_ARG: max_index, B or nnz are
 *                          not the recorded ones, or a valued loc with a binary batch.  The
 *                          Localizer's own carried state (workspace hints, fitted key range,
 *                          hot-key map) is not touched by a replayed step: the next batch that
 *                          runs the lane uses the state of the last batch that ran it, which is
 *                          allowed because the Localizer's outputs are the same bits on every
 *                          path it may choose
 *   dfx_batchcache_stats_loc   out[3] = {batches holding outputs (sealed lists), the bytes they
 *                          take (rounded to 256 per array), steps dfx_train_step_loc served
 *                          from outputs of this cache} */
typedef struct {
  const uint64_t* uniq;      /* [U]; NULL: the batch holds no outputs */
  const uint32_t* segstart;  /* [U + 1] */
  const uint32_t* occ_row;   /* [nnz] */
  const float* occ_x;        /* [nnz] (form 1) */
  const uint32_t* rowof;     /* [2 nnz] (form 2) */
  const uint32_t* choff;     /* [U] (n_chunks > 0) */
  const uint32_t* chunk_seg; /* [n_chunks] */
  const uint32_t* totals;    /* device: {U, n_chunks, gate, 0} */
  int64_t U, n_chunks, size, nnz;
  uint64_t max_index;
  int32_t form;              /* 0 binary, 1 valued with occ_x, 2 valued with rowof */
  int32_t reserved;
  int64_t* served;           /* the owning cache's count of steps served */
} dfx_loc;
int dfx_batchcache_append_loc(dfx_batchcache* bc, int* kept);
int dfx_batchcache_get_loc(dfx_batchcache* bc, int64_t list, int64_t i, dfx_loc* out);
int dfx_batchcache_stats_loc(dfx_batchcache* bc, int64_t* out); /* out[3] */
int dfx_train_step_loc(dfx_ctx* ctx, const dfx_batch* batch, const dfx_loc* loc, int job_type,
                       int push_cnt, uint64_t max_index, float* pred_out);

/* ---- a fresh shuffle of a cached list per epoch (difacto_amd/csrc/reshuffle.hip) -----------
 * The cache replays a part's batches as recorded, the same rows in the same batches in every
 * epoch.  The reference's BatchReader shuffles with the process-wide rand() state, which is never
 * reseeded (src/reader/batch_reader.cc:38-45), so its epochs see other batch compositions.  A
 * reshuffler hands out, per epoch, the N rows of a SEALED list (the concatenation of its batches
 * in order) in the order of a keyed bijection of [0, N) (csrc/reshuffle.h: rs_perm, a Feistel
 * network with cycle walking, computed per row on the device — no permutation array, no sort, no
 * host list), cut every batch_rows rows; the last batch holds the remainder.  A destination
 * batch has value iff some batch of the list has, and a binary source reads as ones
 * (dfx_gather_rows_valued's rule); the same for weight: absent reads as 1.0f.  The sources are
 * only read: after any number of epochs the cached batches are the bytes they were.
 *   dfx_reshuffle_create      a device table of the batches' five pointers and their row prefix,
 *                             12 bytes a row of per-epoch scratch and a ring of nring (2..8)
 *                             destination batches, all out of the cache's budget, every array on
 *                             a 256-byte boundary; *kept = 1.  What does not fit the budget (or
 *                             hipMalloc out of memory): *kept = 0, *out = NULL with DFX_OK, the
 *                             cache untouched — training never fails because this could not grow
 *   dfx_reshuffle_begin_epoch on the context's input stream: one kernel computes for every output
 *                             position its source row (rs_perm, a bisection of the row prefix)
 *                             and that row's length, a scan per output batch gives every row's
 *                             offset inside its batch and the batch's nnz, which go to a pinned
 *                             host array; the host waits for them ONCE per epoch (dfx_batch.nnz
 *                             is a host value), never per batch.  *n_batches = ceil(N /
 *                             batch_rows).  A ring whose nnz capacity (it starts at 1.25 times
 *                             the mean batch) is below this epoch's largest batch is regrown here,
 *                             after the ring's `consumed` events, inside the budget; if it no
 *                             longer fits, *n_batches = -1 (DFX_OK) and the caller replays the
 *                             list as recorded (a later begin_epoch tries again)
 *   dfx_reshuffle_next        the input stream waits for the ring entry's `consumed` event (a
 *                             stream wait: the host never blocks), then ONE launch, a wave per
 *                             row, recomputes each row's source and moves its ids, values, label
 *                             and weight and writes the rebased offsets.  *has = 0 past the last
 *                             batch.  The batch is ready by the input stream's order, as a text
 *                             feed's, and stays valid until nring - 1 further batches were taken
 *   dfx_reshuffle_consumed    after the dfx_train_step that took the batch: records the ring
 *                             entry's event on the context stream (as dfx_textfeed_consumed)
 *   dfx_reshuffle_stats       out[4] = {N, batches per epoch, the ring's bytes, the table's and
 *                             the scratch's bytes}
 *   dfx_reshuffle_destroy     joins the device; must come before the cache's own destroy
 *                             (dfx_batchcache_destroy with a live reshuffler is DFX_ERR_ARG)
 * key: any 64 bits; rs_epoch_key(shuffle_seed, epoch, list) is the driver's.  The same key gives
 * the same batches.  DFX_ERR_ARG: an open, dropped or unknown list, N >= 2^31, batch_rows <= 0,
 * nring outside 2..8, next before begin_epoch (or after one that returned -1), consumed with no
 * batch handed out; a rejected call queues nothing. */
typedef struct dfx_reshuffle dfx_reshuffle;
int dfx_reshuffle_create(dfx_batchcache* bc, int64_t list, int64_t batch_rows, int nring,
                         dfx_reshuffle** out, int* kept);
int dfx_reshuffle_destroy(dfx_reshuffle* rs);
int dfx_reshuffle_begin_epoch(dfx_reshuffle* rs, uint64_t key, int64_t* n_batches);
int dfx_reshuffle_next(dfx_reshuffle* rs, dfx_batch* batch, int* has);
int dfx_reshuffle_consumed(dfx_reshuffle* rs);
int dfx_reshuffle_stats(dfx_reshuffle* rs, int64_t* out); /* out[4] */

/* ---- a fresh negative down-sample per reshuffled epoch (difacto_amd/csrc/reshuffle.hip) -----
 * A reader with neg_sampling < 1 decides once which negative rows it drops, and a cache that
 * recorded its batches replays those survivors in every epoch; the reference makes a reader per
 * part per epoch over a rand_r sequence that is never reseeded, so each of its epochs trains on
 * another sample.  Over a list that holds EVERY row (recorded with neg_sampling 1),
 *   dfx_reshuffle_begin_epoch_sampled
 * opens an epoch as dfx_reshuffle_begin_epoch does, the rows in the order of rs_perm under `key`,
 * without the rows rs_dropped(key, source row, label, neg_sampling) names (csrc/reshuffle.h: the
 * reader's own inequality, label <= 0 and u > 1 - neg_sampling in fp32, u = rs_draw(key, source
 * row) a keyed draw per SOURCE row; it drops a negative with probability neg_sampling, as the
 * reference does).  On the context's input stream: a kernel computes every position's source,
 * length and keep flag, a multi-launch scan of the flags (per-tile counts, one block over the
 * tiles, per-tile ranks: the order is the scan's, never an atomic ticket's) compacts the kept
 * rows' sources and lengths in permuted order, and the per-batch scan runs over the K kept rows,
 * cut every batch_rows of them.  The per-batch nnz and K go to the pinned array and the host
 * waits ONCE.  *n_batches = ceil(K / batch_rows), *n_rows = K; K = 0 is legal (*n_batches = 0,
 * the first dfx_reshuffle_next gives *has = 0).  dfx_reshuffle_next then copies by the compacted
 * sources (one launch a batch, a wave a row, the same ring, events, value and weight rules), and
 * dfx_reshuffle_consumed is as above.  The compacted arrays, 8 bytes a row (and 4 per 2048 rows),
 * are taken from the cache's budget at the first call, on 256-byte boundaries, and counted in
 * dfx_reshuffle_stats' scratch from then on; if they do not fit, or the ring cannot be regrown,
 * *n_batches = -1 (DFX_OK), the cache untouched, and dfx_reshuffle_begin_epoch still works.
 * neg_sampling >= 1 drops nothing: the epoch's batches are dfx_reshuffle_begin_epoch's bit for
 * bit.  Sampled and plain epochs may alternate.  DFX_ERR_ARG: a null argument, a NaN or negative
 * neg_sampling; a rejected call queues nothing. */
int dfx_reshuffle_begin_epoch_sampled(dfx_reshuffle* rs, uint64_t key, float neg_sampling,
                                      int64_t* n_batches, int64_t* n_rows);

/* ---- prediction rows as text on the device (difacto_amd/csrc/predtext.hip) ----------------
 * SGDLearner::SavePred (src/sgd/sgd_learner.h:72-83) writes one line per row,
 *   label '\t' (pred_prob ? 1 / (1 + exp(-pred)) : pred) '\n',  both fields as "%g";
 * the driver's host loop prints fprintf("%g\t%g\n", label, pred_prob ? 1.0 / (1.0 +
 * std::exp(-pred)) : (double)pred) with label and pred floats.  dfx_format_pred forms those
 * bytes on the device (csrc/fmtg.h: glibc's expf restated, IEEE double add and divide, %g as
 * integer arithmetic, round half to even on the exact binary value): text_dev[0, bytes) holds
 * the rows' lines in order, identical to the host loop's, for every row whose two fields are
 * +-0 or 1e-12 <= |x| < 1e12 (csrc/fmtg.h widens this a little).  Any other row (non-finite, a
 * probability below 1e-14, ...) is FLAGGED: it contributes no bytes, and the caller has the host
 * write the batch.  stat_dev[4] (device) = {bytes written, rows flagged, the first flagged row
 * or -1, bytes the text needs}; [3] > [0] iff cap_bytes was too small: the text is then cut at
 * cap_bytes and no byte at or past it is written.  26 * n bytes always suffice.  value_out
 * (optional, device, n doubles): the double each row's second field printed.  Three launches
 * and a one-thread init on the context stream (rows to 32-byte records and tile totals, one
 * block over the totals, the write pass); nothing waits on another block.  Scratch is the
 * context's (32 bytes a row, grow-only; growing may synchronise).  DFX_ERR_ARG, nothing queued:
 * a null ctx or stat_dev, n < 0 or n > 2^26, null label / pred / text with n > 0, cap_bytes < 0.
 *
 * A dfx_predtext double-buffers that for a prediction pass: two slots of device text, pinned
 * host text and pinned copies of the batch's labels and predictions (what the host loop needs
 * when a row was flagged).
 *   dfx_predtext_submit   slot 0 | 1, not pending: on the context stream, so behind the step
 *                         that wrote pred_dev, formats the n rows into the slot, then queues the
 *                         copies down and the slot's event.  The slot grows to n rows on demand
 *                         (that may synchronise).  label_dev and pred_dev are free for reuse by
 *                         later work on the context stream.
 *   dfx_predtext_take     waits for that slot's event alone and hands out the pinned text and
 *                         arrays, valid until the slot's next submit; the slot is free again.
 *                         Slot t is written to the file while the step of t + 1 runs.
 *   dfx_predtext_destroy  joins the context stream.
 * DFX_ERR_ARG: a slot outside 0..1, submit on a pending slot, take on one that is not, n as
 * above; a rejected call queues nothing. */
typedef struct dfx_predtext dfx_predtext;
typedef struct dfx_predtext_out {
  const char* text;  /* pinned: bytes of text */
  int64_t bytes, rows;
  int64_t flagged, first_flagged; /* rows the device did not format; the first, or -1 */
  const float* label; /* pinned: the batch's labels and raw predictions, rows each */
  const float* pred;
} dfx_predtext_out;
int dfx_format_pred(dfx_ctx* ctx, const float* label_dev, const float* pred_dev, int64_t n,
                    int pred_prob, char* text_dev, int64_t cap_bytes, int64_t* stat_dev,
                    double* value_out);
int dfx_predtext_create(dfx_ctx* ctx, int64_t rows_hint, dfx_predtext** out);
int dfx_predtext_submit(dfx_predtext* pt, int slot, const float* label_dev, const float* pred_dev,
                        int64_t n, int pred_prob);
int dfx_predtext_take(dfx_predtext* pt, int slot, dfx_predtext_out* out);
int dfx_predtext_destroy(dfx_predtext* pt);

/* ---- Localizer::Compact (localizer.h:41-51) -------------------------------------------
 * keys = ReverseBytes(index % max_index); uniq[U] ascending, cnt[U] occurrence counts
 * (float, may be NULL), col[nnz] = rank of each nnz's key (the u32 CSR index).  Offsets,
 * values and labels of the compacted block equal the input's (every index matches).
 * uniq and cnt need room for nnz entries.  *n_uniq receives U (synchronises). */
int dfx_localize(dfx_ctx* ctx, int64_t B, int64_t nnz, const uint64_t* offset,
                 const uint64_t* index, uint64_t max_index, uint64_t* uniq, float* cnt,
                 uint32_t* col, int64_t* n_uniq);
/* The Localizer as dfx_train_step's lane and dfx_split_owner_begin run it (no col; the bucket
 * sort unless loc_bucket=0 or its hints choose the radix sort), with the long segments' chunk
 * plan, on the context's main lane — whose hints and device state carry from call to call as a
 * lane's do in training — then copied out; synchronises.  For tests: the fused step reads
 * these arrays in place.  value NULL: binary.  keys_ready: index holds the final keys (the
 * split owner's form; max_index ~0).  Device buffers: uniq[nnz], segstart[nnz + 1],
 * occ_row[nnz], occ_x[nnz] (valued), choff[nnz], chunk_seg[nnz / 128 + nnz / 129 + 2],
 * rowof[2 * nnz] (valued).  Written: uniq[U] ascending, segstart[U + 1], per occurrence in
 * (key, position) order its row and value; when the plan holds chunks, choff[U] (a segment's
 * first chunk) and chunk_seg[n_chunks].  With lb_gather=2 a valued bucket batch leaves each
 * occurrence's input position in occ_row and {row, value bits} by position in rowof
 * (stats[10] = 1), as the backward reads them; occ_x is then not written.
 * stats[16] (host): U, n_chunks, the plan's gate, 1 when the bucket sort ran, the
 * workspace's four hint words (oversize buckets of its last bucket sort, radix sorts since,
 * item form 1 packed / 2 not, hot-key map built), oversize buckets of this batch (bucket sort
 * only), batches placed by the hot-key map so far, rowof written, a key map fitted; of the
 * bucket sort's launch: bucket bits, row tiles, rows per tile, 1 for the unpacked sort form. */
int dfx_localize_occ(dfx_ctx* ctx, int64_t B, int64_t nnz, const uint64_t* offset,
                     const uint64_t* index, const float* value, uint64_t max_index,
                     int keys_ready, uint64_t* uniq, uint32_t* segstart, uint32_t* occ_row,
                     float* occ_x, uint32_t* choff, uint32_t* chunk_seg, uint32_t* rowof,
                     int64_t* stats);

/* ---- FMLoss / LogitLoss ----------------------------------------------------------------
 * weights: the interleaved Pull layout [w | V(V_dim)] addressed by w_pos / V_pos
 * (SGDLearner::GetPos).  V_dim == 0 is LogitLoss; then w_pos may be NULL (w = weights[col]).
 * V_dim > 0 requires w_pos and V_pos.  n_cols = number of columns (U).
 * pred accumulates (+=) like the reference; grad accumulates too (pre-zero it). */
int dfx_fm_predict(dfx_ctx* ctx, int64_t B, int64_t nnz, const uint64_t* offset,
                   const uint32_t* col, const float* value, const float* weights,
                   const int32_t* w_pos, const int32_t* V_pos, int64_t n_cols, int V_dim,
                   float* pred);
int dfx_fm_calcgrad(dfx_ctx* ctx, int64_t B, int64_t nnz, const uint64_t* offset,
                    const uint32_t* col, const float* value, const float* label,
                    const float* row_weight, const float* weights, const int32_t* w_pos,
                    const int32_t* V_pos, int64_t n_cols, int V_dim, const float* pred,
                    float* grad);
/* SGDLearner::GetPos: lens[n] -> w_pos[n], V_pos[n] */
int dfx_get_pos(dfx_ctx* ctx, int64_t n, const int32_t* lens, int32_t* w_pos, int32_t* V_pos);
/* Loss::Evaluate and BinClassMetric::AUC (returns AUC*n like the reference) */
int dfx_evaluate(dfx_ctx* ctx, int64_t B, const float* label, const float* pred, double* objv);
int dfx_auc(dfx_ctx* ctx, int64_t B, const float* label, const float* pred, double* auc_n);

/* ---- Store / SGDUpdater (device hash table, lazy V pool) --------------------------------
 * keys: n reversed feature ids, unique within one call (the Localizer guarantees it).
 * pull: vals needs room for n*(1+V_dim); lens (n, NULL when V_dim == 0) receives 1 or
 *       V_dim+1; *n_vals the number of values written (synchronises).
 * push: DFX_FEA_COUNT (vals[n]) or DFX_GRADIENT (interleaved like pull; lens NULL means
 *       w only).  Processing order = array order (InitV draws rand_r in that order). */
int dfx_store_pull(dfx_ctx* ctx, const uint64_t* keys, int64_t n, float* vals, int32_t* lens,
                   int64_t* n_vals);
int dfx_store_push(dfx_ctx* ctx, const uint64_t* keys, int64_t n, int type, const float* vals,
                   int64_t n_vals, const int32_t* lens);
int dfx_store_save(dfx_ctx* ctx, const char* path, int save_aux);
int dfx_store_load(dfx_ctx* ctx, const char* path);
/* only the keys rank `rank` of `nranks` owns in the sharded store (floor(key·nranks/2^64)):
 * a model saved by N servers (<prefix>_part-<r>, r < N) loads into M servers by every server
 * loading every part */
int dfx_store_load_part(dfx_ctx* ctx, const char* path, int rank, int nranks);
int dfx_store_dump(dfx_ctx* ctx, const char* path, int dump_aux, int need_reverse);

/* ---- model files written from the device (difacto_amd/csrc/modelfile.hip) ------------------
 * The same two files as dfx_store_save and dfx_store_dump above, byte for byte, without the
 * table crossing to the host slot by slot:
 *   SGDUpdater::Save  src/sgd/sgd_updater.h:96-106 with SGDEntry::SaveEntry :35-48: per entry
 *                     key(8) int size(4) w(4) [sqrt_g z] [V(d)] [Vaux(d)], an entry with
 *                     w == 0.f and no V (SGDEntry::empty()) left out; one bool in front
 *   SGDUpdater::Dump  src/sgd/sgd_updater.h:108-139: per entry the line
 *                     key \t size \t w [\t sqrt_g \t z] [\t V..] [\t Vaux..] \n through
 *                     operator<<, the key nibble-reversed first under need_reverse
 * in the table's slot order, the host writers' order.  Floats print through csrc/fmtg.h, which
 * is glibc's %g at precision 6 for +-0 and 1e-12 <= |x| < 1e12 (and answers for 1e-14 <= |x|);
 * anything else - non-finite values, float subnormals, magnitudes outside - the device does
 * not print: it flags the entry, and the chunk is written by the host loop in its place.
 *
 * dfx_model_pack / dfx_model_format run one chunk, slots [slot0, slot0 + nslots) of the table
 * (dfx_store_probe_stats gives its capacity), into caller memory on the context stream.
 * out_dev: device memory, dword aligned; no byte at or past cap_bytes is written.  stat_dev:
 * four device words, final once the stream has passed the call:
 *   [0] bytes the chunk needs   [1] bytes written (min of need and cap_bytes)
 *   [2] entries in the chunk    [3] entries with a field the device did not format (format
 *                                   only; when not 0 the text is not to be used)
 * DFX_ERR_ARG: slots outside the table, cap_bytes < 0, out_dev not aligned, or nslots times
 * the longest record / line for this V_dim beyond 32-bit offsets; a rejected call queues
 * nothing.
 *
 * dfx_store_save_dev / dfx_store_dump_dev write the whole file: two staging buffers with pinned
 * mirrors, chunk t + 1's kernels and chunk t's copy running while the host hands chunk t - 1
 * to one fwrite.  chunk_slots = 0 takes the default, a fixed staging budget (64 MB a buffer)
 * divided by the longest record or line for this V_dim; a larger request is cut to that, so
 * device and pinned memory do not depend on the table's size.  The buffers are made by the
 * context's first such call and kept for its next (freed with the context).  stats (may be
 * NULL): [0] entries written, [1] the file's bytes, [2] chunks, [3] chunks written by the host
 * loop (always 0 for save).  times (may be NULL): the host seconds this call [0] waited for a
 * chunk and [1] spent writing (fwrite, a host-written chunk's loop, fclose).  They return with
 * the file closed and the stream idle. */
int dfx_model_pack(dfx_ctx* ctx, int64_t slot0, int64_t nslots, int save_aux, char* out_dev,
                   int64_t cap_bytes, int64_t* stat_dev);
int dfx_model_format(dfx_ctx* ctx, int64_t slot0, int64_t nslots, int dump_aux, int need_reverse,
                     char* out_dev, int64_t cap_bytes, int64_t* stat_dev);
int dfx_store_save_dev(dfx_ctx* ctx, const char* path, int save_aux, int64_t chunk_slots,
                       int64_t* stats, double* times);
int dfx_store_dump_dev(dfx_ctx* ctx, const char* path, int dump_aux, int need_reverse,
                       int64_t chunk_slots, int64_t* stats, double* times);
int dfx_store_stats(dfx_ctx* ctx, int64_t* n_keys, int64_t* n_vrows, double* new_w,
                    uint32_t* seed);
/* table health: mean and longest distance of a stored key from its home slot; capacity in
 * slots (a test / diagnostics hook) */
int dfx_store_probe_stats(dfx_ctx* ctx, double* mean_probe, int64_t* max_probe,
                          int64_t* capacity);
int dfx_store_evaluate(dfx_ctx* ctx, double* penalty, int64_t* nnz);
int dfx_store_reserve(dfx_ctx* ctx, int64_t n_keys, int64_t n_vrows);
/* test hook: state[4] = {w, sqrt_g, z, fea_cnt}, V/Vaux (2*V_dim floats, host) */
int dfx_store_entry(dfx_ctx* ctx, uint64_t key, float* state, float* V, int* has_v,
                    int* found);

/* ---- fused minibatch (SGDLearner::IterateData executor, sgd_learner.cc:203-269) --------
 * localize -> [push kFeaCount] -> pull -> predict -> evaluate -> AUC -> calcgrad -> push,
 * all on the device with no host round trip.
 * job_type: DFX_JOB_TRAINING updates the model; validation/prediction stop after AUC.
 * push_cnt: push occurrence counts first (epoch 0 with V_dim > 0, sgd_learner.cc:272).
 * pred_out: optional device B floats.  Progress accumulates on the device. */
int dfx_train_step(dfx_ctx* ctx, const dfx_batch* batch, int job_type, int push_cnt,
                   uint64_t max_index, float* pred_out);
int dfx_progress_read(dfx_ctx* ctx, dfx_progress* out, int reset);

/* ---- measurement ------------------------------------------------------------------------
 * HIP events on the context stream around each phase of dfx_train_step, for up to
 * max_steps calls.  dfx_prof_read returns summed ms[7] = {localize (the part of the
 * Localizer lane the context stream waits for), probe + pull, feacnt push, forward,
 * evaluate + AUC snapshot, backward+update, InitV+finalize}, the number of recorded steps,
 * and the mean unique-key count U per step (for algorithmic-byte accounting); it resets. */
int dfx_prof_enable(dfx_ctx* ctx, int max_steps);
/* dfx_prof_enable recording only the marks in mask: bit m (0..7) = the event at the start of
 * phase m (bit 7: the step's end), bit 8 = the lanes' events, bit 9 = the live-V counts of
 * dfx_prof_counts (one extra launch per step).  A phase is timed when both its
 * marks are recorded (0 otherwise); each timing event costs the step a little latency, so a
 * throughput run records only the phase it reports (the backward: bits 5 and 6). */
int dfx_prof_enable_marks(dfx_ctx* ctx, int max_steps, unsigned mask);
int dfx_prof_read(dfx_ctx* ctx, double* ms, int* n_steps, double* mean_u);
/* after dfx_prof_read: out[4] = mean ms per batch of the Localizer lane, of its start and of its
 * end relative to the context stream reaching that batch (start < 0: it ran ahead; end > 0:
 * the exposed wait), and of the AUC lane */
int dfx_prof_lanes(dfx_ctx* ctx, double* out);
/* out[4] = per dfx_train_step since the last call (or dfx_prof_read): the mean number of
 * unique keys, of keys with live V and of their occurrences (the roofline's bytes; the live-V
 * counts are taken only in steps recorded with mark bit 9, dfx_prof_enable_marks); out[3] = the
 * number of batches the bucket Localizer placed by its hot-key map (skewed keys); resets */
int dfx_prof_counts(dfx_ctx* ctx, double* out);
/* out[2] = host seconds dfx_train_step calls spent blocked (the capacity guard waiting for
 * earlier steps' counts) since the last call, and the number of such waits; resets */
int dfx_prof_host(dfx_ctx* ctx, double* out);

/* ---- key-range-sharded store over N GPUs (KVStoreDist, src/store/kvstore_dist.h) --------
 * Every rank is a worker (its own batch) and the server of the keys with
 * floor(key * N / 2^64) == rank.  A step is the sequence below, the collectives in between
 * done by the caller (torch.distributed over RCCL, see difacto_amd/dist.py).  slot (0 or 1)
 * selects one of two sets of step buffers, so that two steps can be in flight: the
 * pipelined schedule issues step t+1's localize / begin / pull before step t's push
 * (dist.py ShardedPipeline); the synchronous schedule can use one slot throughout.
 *   dfx_dist_localize      Localizer::Compact on the Localizer lane (asynchronous): keys_out
 *                          sorted unique keys, cnt_out their occurrence counts (NULL: skip);
 *                          both need room for nnz entries and stay in use until the step's
 *                          dfx_dist_fwd_bwd
 *   dfx_dist_localize_wait host join: split_counts[nranks] the number of keys each rank owns
 *                          (they are contiguous in keys_out), *n_uniq = U
 *   -> alltoallv keys (+ counts) to their owners
 *   dfx_dist_owner_begin   recv_keys: the concatenation of what every rank sent, in rank
 *                          order, recv_offsets[nranks+1] (host) its rank boundaries; with
 *                          recv_cnt the ranks' Update(kFeaCount) pushes in rank order
 *                          (kvstore_dist.h:158-165) and their InitV draws
 *   dfx_dist_owner_pull    Get per received key (kvstore_dist.h:167-175): vals_out[R*S]
 *                          records of S = dfx_dist_record_floats() floats [V | w | live | 0 0]
 *   -> alltoallv records back
 *   dfx_dist_fwd_bwd       forward + Evaluate + AUC of this worker's batch (progress on the
 *                          device), and for training CalcGrad into grads_out[U*S] records
 *                          [gV | gw | live | 0 0] (live: this worker pulled V, the lens of
 *                          its push); pred_out optional device B floats
 *   -> alltoallv gradient records to their owners
 *   dfx_dist_owner_push    the ranks' Update(kGradient) pushes in rank order
 * Owner calls run on the context stream in call order.  All arrays except split_counts /
 * recv_offsets are device pointers. */
int dfx_dist_record_floats(dfx_ctx* ctx);
int dfx_dist_localize(dfx_ctx* ctx, const dfx_batch* batch, uint64_t max_index, int nranks,
                      int slot, uint64_t* keys_out, float* cnt_out);
int dfx_dist_localize_wait(dfx_ctx* ctx, int slot, int nranks, int64_t* split_counts,
                           int64_t* n_uniq);
int dfx_dist_owner_begin(dfx_ctx* ctx, int slot, const uint64_t* recv_keys,
                         const int64_t* recv_offsets, int nranks, const float* recv_cnt);
int dfx_dist_owner_pull(dfx_ctx* ctx, int slot, float* vals_out);
int dfx_dist_fwd_bwd(dfx_ctx* ctx, int slot, const dfx_batch* batch, const float* pulled,
                     int job_type, float* grads_out, float* pred_out);
int dfx_dist_owner_push(dfx_ctx* ctx, int slot, const float* recv_grads);
/* Update aggregation of the sharded store (context kwarg push_agg):
 *   sum (default) — SURVEY §8(e)'s synchronous semantics: a step over N workers is one
 *     reference step (sgd_learner.cc:201-317) on the concatenation of their batches.  The owner
 *     sums the workers' gradient records of a key (rank order) and applies ONE Update
 *     (sgd_updater.cc:76-142); a count push adds the summed counts.  InitV draws are ranked
 *     over all owners in key order, so the rand_r stream is the single updater's: after an
 *     owner_begin with counts, and after every owner_push, each owner calls
 *     dfx_dist_initv_local (its request count -> count_dev, a device int64), the caller
 *     all-gathers the counts (rank order) into counts_all_dev[nranks] (device), and
 *     dfx_dist_initv_draw draws this owner's keys after the lower owners' (rank = this owner's
 *     range).  owner_pull / owner_begin / owner_push refuse to run while that is pending.
 *   ranks — KVStoreDist's HandlePush (kvstore_dist.h:158-165): one Update per pushing worker in
 *     rank order, each server with its own rand_r stream (InitV inside begin / push).
 * dfx_dist_push_agg_sum: 1 for sum, 0 for ranks. */
int dfx_dist_initv_local(dfx_ctx* ctx, int slot, int64_t* count_dev);
int dfx_dist_initv_draw(dfx_ctx* ctx, int slot, const int64_t* counts_all_dev, int rank,
                        int nranks);
int dfx_dist_push_agg_sum(dfx_ctx* ctx);
/* The literal north_star exchange: all-gather of the workers' keys, their
 * sorted union (dfx_dist_union), an all-gather of the owners' union-indexed pull records and a
 * reduce-scatter of union-indexed gradient rows, each owner's chunk of M rows holding its keys
 * in union order (dfx_dist_union_rows maps a worker's rows to and from that layout).  Kept as
 * the measured baseline beside the all-to-all-v schedule; the owner phases are the same
 * (owner_begin over its union slice as one run, push_agg=sum). */
int dfx_dist_union(dfx_ctx* ctx, const uint64_t* runs, const int64_t* run_offs, int nruns,
                   int nranks, uint64_t* union_out, uint32_t* upos_out, int64_t* bounds_out,
                   int64_t* n_union);
int dfx_dist_union_rows(dfx_ctx* ctx, const uint64_t* keys, const uint32_t* upos, int64_t U,
                        const int64_t* bounds, int nranks, int64_t M, int width, int to_union,
                        const float* src, float* dst);

/* ---- owner-computes split of FM over the key-range shards (difacto_amd/csrc/split.hip) -----
 * SURVEY §8(e)'s synchronous step (push_agg=sum: one reference step on the concatenation of the
 * workers' batches, sgd_learner.cc:201-317), with the forward and backward run by the owners of
 * the keys, so only per-row quantities cross the links.  Per step, every rank:
 *   dfx_split_partition      worker: each nnz's key (ReverseBytes(id % max_index), the
 *                            Localizer's) grouped by owner floor(key * N / 2^64), row order kept:
 *                            keys_out[nnz], x_out[nnz] their values (required for valued data;
 *                            binary data given x_out gets 1s), row_cnt_out[N][B]
 *                            nnz per (owner, row); asynchronous on the context stream
 *   dfx_split_partition_wait host join: split_counts[nranks] keys per owner
 *   -> alltoallv keys (+ values) and row counts (B per owner) to the owners; a driver may pad
 *      every worker to the same row count M with empty rows (equal-size collectives)
 *   dfx_split_owner_begin    owner: the received keys / values / row counts, concatenated in
 *                            rank order (rows_per_rank / keys_per_rank: host, per source rank;
 *                            row_cnt is scanned in place); Localizer::Compact of them; push_cnt:
 *                            Update(kFeaCount) of every key, InitV requests pending; a job
 *                            other than training inserts every key (Get's model_[key]).
 *                            lane = 1 (a training step without count push): on the Localizer
 *                            lane (dfx_ctx_lane_stream 0), whose queue the caller made wait for
 *                            the received arrays; it waits for the slot's previous step and
 *                            owner_forward waits for it, so it runs beside the previous step's
 *                            owner_forward / owner_backward on the context stream
 * dfx_split_partition runs on a stream of its own, after the batch's producer (the input
 * stream, dfx_ctx_set_input_stream, else the context stream).
 *   dfx_split_owner_forward  owner: part_out[R][dfx_split_part_floats(ctx, nranks)] per
 *                            received row over this owner's keys: one owner [XV(d) | XXVV(d) |
 *                            sum w x | 0 0 0]; N > 1 owners [XV(d) | sum w x | sum_l XXVV_l | 0 0]
 *   -> alltoallv partials back to the workers (rank-major: owner o's rows at o * part_rows)
 *   dfx_split_combine        worker: pred / p / logloss / AUC of its rows from the owners'
 *                            partials (summed in rank order), progress on the device,
 *                            pxv_out[B][dfx_split_pxv_floats()] rows [XV*p (d) | p | 0 0 0],
 *                            pred_out optional
 *   -> every owner receives every worker's pxv rows, in rank order
 *   dfx_split_owner_backward owner: CalcGrad of its keys over the received rows + one Update per
 *                            key (FTRL / AdaGrad); InitV requests pending
 *   after a count push and after every backward (V_dim > 0): dfx_split_initv_local (this owner's
 *   request count -> count_dev, a device int64), the caller all-gathers the counts in rank order
 *   (device int64[nranks]) and dfx_split_initv_draw draws this owner's keys after the lower
 *   owners', so the rand_r stream is the single updater's.  Owner calls run on the context
 *   stream in call order.  Arrays are device pointers unless noted. */
int dfx_split_part_floats(dfx_ctx* ctx, int nranks);
int dfx_split_pxv_floats(dfx_ctx* ctx);
int dfx_split_partition(dfx_ctx* ctx, int slot, const dfx_batch* batch, uint64_t max_index,
                        int nranks, uint64_t* keys_out, float* x_out, uint32_t* row_cnt_out);
int dfx_split_partition_wait(dfx_ctx* ctx, int slot, int nranks, int64_t* split_counts);
int dfx_split_owner_begin(dfx_ctx* ctx, int slot, const uint64_t* keys, const float* x,
                          uint32_t* row_cnt, const int64_t* rows_per_rank,
                          const int64_t* keys_per_rank, int nranks, int job_type,
                          int push_cnt, int lane);
int dfx_split_owner_forward(dfx_ctx* ctx, int slot, float* part_out);
int dfx_split_combine(dfx_ctx* ctx, int slot, const dfx_batch* batch, const float* parts,
                      int64_t part_rows, int nranks, float* pxv_out, float* pred_out);
int dfx_split_owner_backward(dfx_ctx* ctx, int slot, const float* pxv);
/* sliced forms, so a driver can exchange one slice's rows while the next slice computes:
 * dfx_split_owner_forward_rows  rows [lo, lo + len) of each of the nranks source workers'
 *                               M-row blocks (the received rows must be nranks * M), written
 *                               at their place in part_out; the call ending at M finishes the
 *                               owner's forward (len = 0: all rows, as dfx_split_owner_forward)
 * dfx_split_combine_rows        this worker's rows [lo, lo + len), lo a multiple of 256; the
 *                               call whose rows reach part_rows finishes the step's combine
 *                               (loss, AUC, progress) — as dfx_split_combine over all rows */
int dfx_split_owner_forward_rows(dfx_ctx* ctx, int slot, float* part_out, int nranks, int64_t M,
                                 int64_t lo, int64_t len);
int dfx_split_combine_rows(dfx_ctx* ctx, int slot, const dfx_batch* batch, const float* parts,
                           int64_t part_rows, int nranks, float* pxv_out, float* pred_out,
                           int64_t lo, int64_t len);
/* the owner's last begin: received rows, keys and unique keys (synchronises the stream) */
int dfx_split_owner_stats(dfx_ctx* ctx, int slot, int64_t* rows, int64_t* nnz,
                          int64_t* n_uniq);
int dfx_split_initv_local(dfx_ctx* ctx, int slot, int64_t* count_dev);
int dfx_split_initv_draw(dfx_ctx* ctx, int slot, const int64_t* counts_all_dev, int rank,
                         int nranks);

#ifdef __cplusplus
}
#endif
#endif /* DIFACTO_AMD_H_ */
