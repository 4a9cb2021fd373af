// train_main.cc — dfx_train: the reference's `difacto` executable for the SGD learner
// (src/main.cc + SGDLearner::RunScheduler, src/sgd/sgd_learner.cc:51-117) on one GPU.
//
//   build/dfx_train data_in=FILE [data_val=FILE] [data_format=libsvm|criteo|criteo_test|adfea]
//                   [batch_size=100] [shuffle=10] [neg_sampling=1] [max_num_epochs=20]
//                   [num_jobs_per_epoch=10] [stop_rel_objv=1e-5] [stop_val_auc=1e-5]
//                   [model_in=F] [model_out=F]
//                   [load_epoch=-1] [has_aux=0] [task=0|1|2] [pred_out=F] [pred_prob=1]
//                   [fused=1] [nthreads=8] [parse=host|device|auto|auto-sharded] [parse_adfea=0]
//                   [cache=none|device|auto]
//                   [cache_mb=16384] [cache_loc=0] [epoch_shuffle=0] [shuffle_seed=0]
//                   [epoch_resample=0] [pred_write=host|device] [model_write=host|device]
//                   [name_dump=dump.txt] [need_reverse=0] [dump_aux=0]
//                   [V_dim=..] [lr=..] [l1=..] ... (SGDUpdaterParam)
//
// What each option does is described below.  The rules themselves — which combinations are
// refused, with which message and in which order, and the "parse:" / "cache:" lines — are one
// function, ResolveOptions in train_options.h; the code here reads the RunPlan it fills.
//
// parse=device (data_format=criteo|criteo_test, the single-GPU fused path: training, data_val
// validation and task=2 prediction): the raw text is copied to pinned memory and uploaded, the
// device parses it (dfx_parse_criteo) and forms the batches (DeviceBatchReader,
// device_reader.h) — the same batches, so the same results, as the default parse=host.  With
// any other format, fused=0 or the sharded runs it is an error (exit 2).  A chunk the device
// hands back (needs_host) is parsed by the host; their count is printed per epoch if non-zero.
//
// parse=auto takes the device parser when the format has one (criteo, criteo_test: as above;
// libsvm: dfx_parse_libsvm, values included, the batches valued exactly where BatchReader's
// are) and the run is the single-GPU fused path, else the host reader; one line at the start
// says which and why, e.g. "parse: device (libsvm)" or "parse: host (exchange=split)".
// parse=device keeps its contract: Criteo formats only, anything else is an error.
//
// parse_adfea=1 (with data_format=adfea and parse=auto or parse=auto-sharded; anything else is
// an error, exit 2) makes adfea a format with a device parser (dfx_parse_adfea: binary rows of
// any length, batches handed out unvalued as BatchReader's are), so the two values then treat
// it as they treat libsvm and print "parse: device (adfea)" or "parse: device (adfea, <n>
// shards)".  Default 0: adfea is read by the host reader and the lines say "parse: host
// (data_format=adfea)".
//
// parse=auto-sharded is parse=auto that takes the device parser in the sharded runs too
// (shards=N, shards=-1, WORLD_SIZE > 1; both exchanges; pipelined=0|1; training, data_val
// validation and task=2): every local shard reads its parts with a DeviceBatchReader on a text
// feed of its own (DeviceTextFeed on the shard's context, alive for the run), the same parts,
// chunks and batches as the host reader's, so the same results.  The sharded stores queue a
// step's last reader of its batch one Step call late when pipelined, so a feed batch is marked
// by the runner at that call or at the flush (ShardRunner::Mark), not when it is handed over,
// and the feeds are 4 slots and 4 ring entries deep.  Rank 0 prints "parse: device (<format>,
// <n> shards)" or, for a format with no device parser, "parse: host (data_format=<f>)"; without
// shards the value is parse=auto and prints its line.  cache=device|auto records the feed's
// batches; pred_write=host writes from the chunk's labels the parse copied back, pred_write=
// device reads the device labels before the batch is marked.  Chunks handed back to the host
// parser are summed over shards and ranks and reported by rank 0.  A training epoch that read
// also prints where the device readers' time went.
//
// cache=device (the single-GPU fused path with either parse and any data_format, training and
// data_val validation; the sharded exchange=a2a runs): the first epoch the run executes (after
// load_epoch: not epoch 0) also copies every batch it forms into a device batch cache
// (DeviceBatchCache, gpu_adapters.h; dfx_batchcache_*), one list per job kind and part, within
// cache_mb MB (per shard in a sharded run).  A reader lives for one part of one epoch and seeds
// its shuffle and down-sampling afresh, so a part yields the same batches in every epoch: every
// later epoch steps through the cached batches with no reader, no upload and no parse, and
// computes the same losses and model.  A part whose batches did not fit is read as without the
// cache.  After the recording epoch one line reports the batches and MB held and the parts not
// cached.  With exchange=split or fused=0 it is an error (exit 2); task=2 is one pass over the
// data, so there it is accepted and has no effect.
//
// cache=auto takes the device cache on every path that can replay device batches: the
// single-GPU fused path and exchange=a2a (there it runs as cache=device does) and exchange=split
// (GpuSplitLearner::ProcessDeviceBatches: a replayed batch goes to the split store as it is, a
// part that did not fit is read while the other shards replay); with fused=0 it runs without a
// cache.  One line at the start says which, "cache: device (fused)", "cache: device
// (exchange=a2a)", "cache: device (exchange=split)", "cache: none (fused=0)" or, in the one pass
// of a prediction run, "cache: none (task=2)"; the report line after the recording epoch is
// cache=device's.  An exchange=split run with the cache also prints per epoch where the
// submitting thread's time went.  cache_mb < 0 is an error (exit 2); cache_loc=1 and
// epoch_shuffle=1 ask for cache=device literally.  cache=device keeps its contract: a path
// without the cache is an error.
//
// cache_loc=1 (with cache=device, the single-GPU fused path, not task=2): the recording epoch
// also keeps, next to every cached batch, the outputs of that batch's Localizer
// (dfx_batchcache_append_loc after each step, training and data_val alike), and the replayed
// epochs step from them with no Localizer at all (dfx_train_step_loc) — a batch's Localizer
// output depends on the batch alone, so the losses and the model are the same bits.  It costs
// ~16 B/nnz of the budget where nearly every key of a batch is distinct, beside the batch's
// 8 B/nnz (about three times the cache), far less on skewed data; outputs that do not fit are
// left out and their batches replay with the Localizer.  One more line after the cache's
// reports the batches that hold outputs and their MB.  Without cache=device, with fused=0,
// task=2 or in a sharded run it is an error (exit 2).  Default 0: the run as without it.
//
// epoch_shuffle=1 (with cache=device, the single-GPU fused path, not task=2, not cache_loc=1):
// a reader seeds its shuffle afresh, so a part yields the same rows in the same batches in every
// epoch, cached or not; the reference's BatchReader draws from the process-wide rand() state,
// which is never reseeded (src/reader/batch_reader.cc:38-45), so its epochs see other batch
// compositions.  With this option the recording epoch is unchanged, and in every later epoch each
// TRAINING part whose list is sealed is stepped through a device reshuffler (DeviceReshuffler,
// gpu_adapters.h; dfx_reshuffle_*): all rows of the part in the order of a keyed permutation
// (csrc/reshuffle.h, key = rs_epoch_key(shuffle_seed, epoch, list)), cut into batches of
// batch_size rows, gathered on the device out of the cached batches, which stay as they are.
// Parts run in order and validation lists replay as recorded; a part that is not cached, or whose
// reshuffler did not fit cache_mb, goes the way it goes without the option.  The same
// shuffle_seed gives the same run.  One line after the cache's says how many parts reshuffle and
// the MB their rings and scratch take, and every reshuffled epoch prints the time the host
// waited for the batches' sizes (once per part).  Without cache=device, with cache_loc=1 (new
// batches have no kept Localizer outputs), fused=0, task=2 or in a sharded run it is an error
// (exit 2).  Default 0: the run as without it.
//
// epoch_resample=1 (with epoch_shuffle=1 and neg_sampling < 1): a reader decides once which
// negative rows it drops and the cache records the survivors, so every replayed epoch trains on
// the same sample and a dropped row is never seen; the reference makes a BatchReader per part per
// epoch over a rand_r sequence that is never reseeded, so each of its epochs draws another
// sample.  With this option the TRAINING readers of the recording epoch drop nothing
// (neg_sampling 1), so the cache holds every row; each part is recorded WITHOUT training, its
// list sealed and its reshuffler made, and then, in the recording epoch and in every later one,
// stepped through DeviceReshuffler::BeginEpochSampled under rs_epoch_key(shuffle_seed, epoch,
// list): this epoch's order without the negatives this epoch's keyed draw drops (csrc/reshuffle.h:
// rs_dropped, the reader's own inequality; a negative is dropped with probability neg_sampling, as
// the reference does).  Every epoch, the first included, sees a fresh order and a fresh sample;
// push_cnt stays "epoch 0 of training"; validation readers and lists are as without it.  A part
// whose list was dropped, whose reshuffler did not fit or whose sampled epoch does not fit is
// never stepped unsampled out of the cache: it is read through its reader with the reader's own
// sample (in the recording epoch that is a second read of the part).  One line after the cache's
// and epoch_shuffle's says how many parts resample, and every epoch prints the rows kept of the
// rows held.  Without epoch_shuffle=1, or with neg_sampling >= 1, it is an error (exit 2).
// Default 0: the run as without it.
//
// pred_write=device (task=2 with pred_out; the single-GPU fused path with either parse, and the
// sharded runs with both exchanges): every <pred_out>_part-<rank> is written from text the
// device formatted (DevicePredWriter, gpu_adapters.h; dfx_predtext_*; csrc/fmtg.h restates
// glibc's "%g" and the probability expression, bit for bit) instead of the host's per-row
// fprintf: the predictions stay on the device, a batch's text comes down in one copy and is
// written with one fwrite while the next step runs.  The files are the host writer's byte for
// byte: a batch holding a row the device does not format (a field that is not 0 and outside
// 1e-12 <= |x| < 1e12: a non-finite prediction, a probability below 1e-14) is written whole by
// the host loop (WritePredRows) in its place, and the number of such batches is printed when
// it is not zero.  One line after "Prediction:" gives the rows, the pass's seconds and the
// seconds the host waited for text.  With fused=0, or a value other than host or device, it is
// an error (exit 2, before any context exists); without task=2 it is accepted and does
// nothing.  Default host: the run as without it.
//
// model_write=device (with model_out; the single-GPU run with either fused value, and the
// sharded runs with both exchanges): every <model_out>_part-<rank> is packed on the device
// (GpuSGDUpdater::SaveFile, dfx_store_save_dev; csrc/modelfile.hip) instead of the host's walk
// over a copy of the whole table with a few fwrite calls of 4 to 8 bytes per entry: the table is
// read in chunks of slots where it lies, a chunk's records come down in one copy and are written
// with one fwrite while the next chunk is packed, and in the single-GPU run the file is written
// straight to its path (the default goes through a temporary file and a copy of it in memory).
// The file is the host writer's byte for byte.  One line after the save gives the entries, the
// MB, the seconds and the seconds the host waited for chunks.  A value other than host or device
// is an error (exit 2); without model_out it is accepted and does nothing.  Default host: the
// run as without it.
//
// task=1 (src/main.cc:81-87 with src/reader/dump.h) dumps a model as text: model_in, the literal
// file (not a prefix: dump.h:55-56 opens it as it is named), is loaded (V_dim as for task=2; a
// mismatch is the loader's error) and written to name_dump (default dump.txt) in
// SGDUpdater::Dump's lines, key \t size \t w [\t sqrt_g \t z] [\t V..] [\t Vaux..], the
// bracketed state under dump_aux=1 and the key nibble-reversed back to the feature id under
// need_reverse=1.  data_in is not needed.  model_write names the writer: host is dfx_store_dump's
// loop, device formats the lines on the device (dfx_store_dump_dev; csrc/modeltext.h prints a
// float as operator<< does through csrc/fmtg.h) - the same bytes: a chunk of slots holding a
// float the device does not format (not finite, a float subnormal, outside 1e-14 <= |x| < 1e12)
// is written by the host loop in its place, and the count of such chunks is printed when it is
// not zero.  It prints "Dump: <entries> entries, <bytes> bytes in <s> s".  Without model_in
// ("dump needs model_in") or in a sharded invocation it is an error (exit 2).
//
// Sharded store (KVStoreDist over GPUs, dist_host.h): `shards=N` holds N shards on this GPU
// (loopback exchange, for tests); `shards=-1` or a launch with WORLD_SIZE > 1 (RANK / LOCAL_RANK as
// torchrun sets them; DFX_COMM_ID_FILE or /tmp/dfx_comm_<MASTER_PORT> as the node-local
// rendezvous) runs one shard per process over RCCL.  Every epoch is split into
// num_jobs_per_epoch x shards parts; shard r reads parts r, r + shards, ... in order, the shards
// step together (an exhausted shard submits empty batches until all are done), and
// `pipelined=1` (default) selects the 1-step-stale schedule.  Each server saves
// <model_out>_part-<rank>; `model_in_parts=K` loads a model K servers saved into this run's
// shards (each keeps the keys it owns).  `exchange=split` runs the sharded epochs through the
// owner-computes split (GpuSplitLearner, split_learner.h) instead of KVStoreDist's exchanges.
// Both exchanges run the same epoch loop (ShardedPass over a ShardRunner).  With data_val every
// epoch ends in a validation pass: the store is flushed first (the stale schedule's last push is
// applied), the shard of rank g reads part j * shards + g of data_val as whole 256 MB chunks,
// one batch per chunk, the shards stepping together as in training; rank 0 prints the
// "Epoch[k] Validation:" line from the all-reduced sums, and the stop rules (training loss, then
// validation AUC against stop_val_auc, sgd_learner.cc:92-106) are decided on those sums, the
// same on every rank.  task=2 (needs model_in and data_val, else exit 2) is one such pass with
// job type prediction: every rank writes <pred_out>_part-<its global rank>, one
// "label\tprediction" line per row in the order it read them (the file exists even when it read
// none), and rank 0 prints the "Prediction:" line.  A prediction step runs synchronously
// (submit, flush, copy the predictions down); validation steps are queued like training steps.
// cache=device exchange=a2a and cache=auto keep and replay the validation batches too (lists of
// their own).
//
// Model files are named like SGDLearner::ModelName (sgd_learner.h:65-69):
// <prefix>[_iter-<epoch>]_part-0, in SGDUpdater::Save's format; task=2 predicts data_val with
// model_in into <pred_out>_part-0, one "label\tprediction" line per row (SavePred,
// sgd_learner.h:72-83).
//
// Each epoch reads data_in in num_jobs_per_epoch parts (the reference's jobs, here run in
// order), minibatched by BatchReader (reader.h) and trained through GpuSGDLearner, i.e. one
// dfx_train_step per batch behind a pinned-staging dfx_feeder.  It prints the reference's
// "Epoch[k] Training: Rows = .., loss = .., AUC = .." line per epoch, plus the rate including
// parsing and PCIe (host ex/s), which is NOT the device-resident rate bench.py reports.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
#include <string>

#include "../csrc/reshuffle.h"
#include "device_reader.h"
#include "dist_host.h"
#include "gpu_adapters.h"
#include "reader.h"
#include "split_learner.h"
#include "train_options.h"

using namespace difacto;

namespace {
// sgd_learner.h:65-69
std::string ModelNamePart(const std::string& prefix, int iter, int rank) {
  std::string name = prefix;
  if (iter >= 0) name += "_iter-" + std::to_string(iter);
  return name + "_part-" + std::to_string(rank);
}
std::string ModelName(const std::string& prefix, int iter) {  // one server: rank 0
  return ModelNamePart(prefix, iter, 0);
}

double Now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// sgd_utils.h:59-63
std::string Text(const Progress& p) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "Rows = %.0f, loss = %.9g, AUC = %.9g", p.nrows,
                p.loss / p.nrows, p.auc / p.nrows);
  return buf;
}

// pred_write=device, after the "Prediction:" line: what the device writer did (a sharded run:
// this process's shards)
void PrintPredWriteLine(const DevicePredWriter::Stats& st, double pass_s) {
  std::printf("pred_write=device: %lld rows, pass %.3f s, the host waited %.3f s for text\n",
              (long long)st.rows, pass_s, st.wait_s);
  if (st.host_batches)
    std::printf("pred_write=device: %lld batch%s written by the host (a row outside the device "
                "formatter's domain)\n",
                (long long)st.host_batches, st.host_batches == 1 ? "" : "es");
}

// model_write=device, after the save: what the device writer did (a sharded run: this process's
// shards)
void PrintModelWriteLine(const ModelWriteStats& st, double seconds) {
  std::printf("model_write=device: %lld entries, %.1f MB in %.3f s, the host waited %.3f s for "
              "chunks\n",
              (long long)st.entries, (double)st.bytes / (1 << 20), seconds, st.wait_s);
}

// the batch cache's list of a part: one per (job kind, part)
int64_t CacheList(const Param& P, bool train, int part) {
  return (int64_t)(train ? 0 : 1) * P.num_jobs_per_epoch + part;
}

// after the recording epoch: what the batch cache holds (a sharded run: summed over the shards)
void PrintCacheLine(double batches, double bytes, double dropped, double parts) {
  std::printf("cache=device: %.0f batches, %.1f MB held, %.0f of %.0f parts not cached\n", batches,
              bytes / (1 << 20), dropped, parts);
}

// stop criteria (sgd_learner.cc:89-108) on an epoch's sums: the training loss's relative change,
// then the validation AUC's gain; an epoch that does not stop becomes the next one's "pre"
bool ShouldStop(const Progress& tr, const Progress& va, double* pre_loss, double* pre_val_auc,
                const Param& P, bool say) {
  double eps = std::fabs(tr.loss - *pre_loss) / *pre_loss;
  if (eps < P.stop_rel_objv) {
    if (say) std::printf("Change of loss [%g] < stop_rel_objv [%g]\n", eps, P.stop_rel_objv);
    return true;
  }
  if (va.auc > 0) {
    eps = (va.auc - *pre_val_auc) / va.nrows;
    if (eps < P.stop_val_auc) return true;
  }
  *pre_loss = tr.loss;
  *pre_val_auc = va.auc;
  return false;
}

// a part's device reader: training forms minibatches out of 64 MB chunks, shuffled and
// down-sampled; validation and prediction take whole 256 MB chunks, one batch per chunk.
// every_row: a training reader that drops no negative (epoch_resample=1's recording pass)
std::unique_ptr<DeviceBatchReader> MakeDeviceReader(const Param& P, DeviceTextFeed* feed,
                                                    bool train, int part, int nparts,
                                                    bool every_row = false) {
  return std::unique_ptr<DeviceBatchReader>(new DeviceBatchReader(
      feed, train ? P.data_in : P.data_val, P.data_format, part, nparts, train ? P.batch_size : 0,
      train ? P.batch_size * P.shuffle : 0, train && !every_row ? P.neg_sampling : 1.f,
      P.nthreads, train ? (size_t)64 << 20 : (size_t)256 << 20));
}

// what a RunEpoch pass may use (null: not in this run) and what it reports (accumulated)
struct PassIO {
  DeviceTextFeed* feed = nullptr;  // parse=device: the parts are read by a DeviceBatchReader
  // record: the recording pass, every batch is also appended to its part's list (the step still
  // takes the original batch); else a part whose list was sealed is replayed from the cache
  // with no reader, any other part is read as without the cache
  DeviceBatchCache* cache = nullptr;
  bool record = false;
  std::vector<std::unique_ptr<DeviceReshuffler>>* resh = nullptr;  // epoch_shuffle=1: per part
  FILE* pred_file = nullptr;               // prediction: the rows, written by the host loop
  DevicePredWriter* dev_writer = nullptr;  // ... or from text the device formatted
  DeviceBatchReader::Times times;          // the device readers'
  double step_s[2] = {0, 0};        // inside dfx_train_step calls; the parts' final joins
  double shuffle_wait[2] = {0, 0};  // the host's wait for the batches' sizes; parts reshuffled
  // epoch_resample=1: the rows kept of the rows held in the parts resampled; parts read through
  // their readers (a dropped list, a reshuffler or a sample that did not fit)
  int64_t resample_rows[2] = {0, 0};
  int resample_read = 0;
};

// one RunEpoch call, as the four sources of a part's batches see it
struct Pass {
  GpuSGDLearner* learner;
  const Param& P;
  const RunPlan& plan;
  int job_type;
  bool train, push_cnt;
  PassIO* io;
  std::vector<real_t> pred;  // a batch's predictions, where the host loop writes them
  size_t fallback = 0;       // chunks the device handed back to the host parser
  std::vector<real_t>* host_pred() { return io->pred_file && !io->dev_writer ? &pred : nullptr; }
};

// epoch_shuffle=1: the part's rows in this epoch's order, gathered out of the cached batches
void StepReshuffled(Pass* s, DeviceReshuffler* rs) {
  dfx_batch b;
  while (rs->Next(&b)) {
    const double ts = Now();
    s->learner->ProcessDeviceBatch(b, s->job_type, s->push_cnt);
    rs->Consumed();
    s->io->step_s[0] += Now() - ts;
  }
  s->io->shuffle_wait[1] += 1;
}

// a sealed list's n batches as they were recorded (cache_loc=1: with their Localizer outputs)
void StepReplayed(Pass* s, int64_t list, int64_t n) {
  DeviceBatchCache* cache = s->io->cache;
  for (int64_t i = 0; i < n; ++i) {
    const dfx_batch b = cache->Get(list, i);
    dfx_loc loc;
    if (s->plan.cache_loc) loc = cache->GetLoc(list, i);
    const double ts = Now();
    s->learner->ProcessDeviceBatch(b, s->job_type, s->push_cnt, nullptr,
                                   s->plan.cache_loc ? &loc : nullptr);
    s->io->step_s[0] += Now() - ts;
  }
}

// parse=device: the same parts, chunks and batches, formed on the device
void StepDeviceReader(Pass* s, int part, bool rec) {
  PassIO& io = *s->io;
  const auto reader = MakeDeviceReader(s->P, io.feed, s->train, part, s->P.num_jobs_per_epoch);
  while (reader->Next()) {
    const dfx_batch& b = reader->Value();
    if (rec) io.cache->Append(b);
    const double ts = Now();
    const float* dpred = nullptr;
    s->learner->ProcessDeviceBatch(b, s->job_type, s->push_cnt, s->host_pred(), nullptr,
                                   io.dev_writer ? &dpred : nullptr);
    // (before Consumed: the ring entry's labels are read behind the step)
    if (io.dev_writer) io.dev_writer->Submit(b.label, dpred, b.size);
    reader->Consumed();
    io.step_s[0] += Now() - ts;
    if (rec && s->plan.cache_loc) io.cache->AppendLoc();
    if (s->host_pred())
      WritePredRows(io.pred_file, reader->HostLabels(), s->pred.data(), s->pred.size(),
                    s->P.pred_prob);
  }
  s->fallback += reader->FallbackChunks();
  io.times += reader->TimesSpent();
}

// the host readers behind the pinned-staging feeder
void StepHostReader(Pass* s, int part, bool rec) {
  const Param& P = s->P;
  PassIO& io = *s->io;
  const bool rec_loc = rec && s->plan.cache_loc;  // each step's Localizer outputs with its batch
  if (s->train) {
    // sgd_learner.cc:273-280
    ThreadedBatchReader reader(P.data_in, P.data_format, part, P.num_jobs_per_epoch, P.batch_size,
                               P.batch_size * P.shuffle, P.neg_sampling, P.nthreads);
    while (reader.Next()) {
      const auto blk = reader.Value().GetBlock();
      dfx_batch db;
      s->learner->ProcessBatch(blk, s->job_type, s->push_cnt, nullptr, rec ? &db : nullptr);
      if (rec) io.cache->Append(db);
      if (rec_loc) io.cache->AppendLoc();
    }
    return;
  }
  // sgd_learner.cc:281-286: validation reads whole 256 MB chunks as one batch
  TextReader reader(P.data_val, P.data_format, part, P.num_jobs_per_epoch, 256 << 20, P.nthreads);
  while (reader.Next()) {
    const auto& v = reader.Value();
    if (v.Size() == 0) continue;
    dfx_batch db;
    const float* dpred = nullptr;
    s->learner->ProcessBatch(v.GetBlock(), s->job_type, false, s->host_pred(),
                             rec || io.dev_writer ? &db : nullptr,
                             io.dev_writer ? &dpred : nullptr);
    if (rec) io.cache->Append(db);
    if (rec_loc) io.cache->AppendLoc();
    // (the feeder's slot of this batch is uploaded into again two batches on; the writer is
    // done reading a batch when the next Submit returns)
    if (io.dev_writer) io.dev_writer->Submit(db.label, dpred, db.size);
    if (s->host_pred())
      WritePredRows(io.pred_file, v.label.data(), s->pred.data(), s->pred.size(), P.pred_prob);
  }
}

// epoch_resample=1, the recording pass of a training part: every row of the part (the reader
// drops none) into the open list, and no step.  No step marks a batch consumed, so the host
// waits for the input stream, where the batch was produced and copied, before its producer
// takes the buffers back.
void RecordPart(Pass* s, int part) {
  const Param& P = s->P;
  PassIO& io = *s->io;
  if (io.feed) {
    const auto reader = MakeDeviceReader(P, io.feed, true, part, P.num_jobs_per_epoch, true);
    while (reader->Next()) {
      io.cache->Append(reader->Value());
      DfxCheck(dfx_sync_input(s->learner->context()), "dfx_sync_input");
      reader->Consumed();
    }
    s->fallback += reader->FallbackChunks();
    io.times += reader->TimesSpent();
    return;
  }
  ThreadedBatchReader reader(P.data_in, P.data_format, part, P.num_jobs_per_epoch, P.batch_size,
                             P.batch_size * P.shuffle, 1.f, P.nthreads);
  while (reader.Next()) {
    io.cache->Append(s->learner->UploadBatch(reader.Value().GetBlock()));
    s->learner->UploadDone();
  }
}

// epoch_resample=1, a training part: in the recording epoch its rows are recorded first and its
// reshuffler made; then, in every epoch, the part is stepped through this epoch's order and this
// epoch's sample of the cached rows.  A part that cannot be (its list was dropped, its
// reshuffler or the sample's scratch did not fit) is read through its reader with the reader's
// own sampling, never stepped unsampled out of the cache.
void StepResampled(Pass* s, int epoch, int part) {
  const Param& P = s->P;
  PassIO& io = *s->io;
  const int64_t list = CacheList(P, true, part);
  std::unique_ptr<DeviceReshuffler>& rs = (*io.resh)[(size_t)part];
  if (io.record) {
    io.cache->Begin(list);
    RecordPart(s, part);
    if (io.cache->Seal() >= 0) {
      rs.reset(new DeviceReshuffler(io.cache, list, (int64_t)P.batch_size, 4));
      if (!rs->kept()) rs.reset();
    }
  }
  int64_t n = -1, rows = 0;
  if (rs) {
    const double tb = Now();
    n = rs->BeginEpochSampled(rs_epoch_key(P.shuffle_seed, (uint64_t)epoch, (uint64_t)list),
                              P.neg_sampling, &rows);
    io.shuffle_wait[0] += Now() - tb;
  }
  if (n >= 0) {
    StepReshuffled(s, rs.get());
    io.resample_rows[0] += rows;
    io.resample_rows[1] += rs->GetStats().rows;
    return;
  }
  // the sample's scratch or the ring did not fit while the part was recorded: the part reads
  // through its reader in every epoch, its reshuffler's memory goes back to the cache, and the
  // line after the cache's counts it among the parts read
  if (rs && io.record) rs.reset();
  io.resample_read += 1;
  if (io.feed)
    StepDeviceReader(s, part, false);
  else
    StepHostReader(s, part, false);
}

Progress RunEpoch(GpuSGDLearner* learner, const Param& P, const RunPlan& plan, int epoch,
                  int job_type, PassIO* io) {
  Progress prog;
  const bool train = job_type == GpuSGDLearner::kTraining;
  Pass s{learner, P, plan, job_type, train, train && epoch == 0, io, {}, 0};
  for (int part = 0; part < P.num_jobs_per_epoch; ++part) {
    if (train && plan.epoch_resample && io->cache) {
      StepResampled(&s, epoch, part);
      const double tj = Now();
      const Progress p = learner->TakeProgress();
      io->step_s[1] += Now() - tj;
      prog.nrows += p.nrows;
      prog.loss += p.loss;
      prog.auc += p.auc;
      continue;
    }
    const int64_t list = CacheList(P, train, part);
    const bool rec = io->cache && io->record;
    const int64_t n_cached = io->cache && !io->record ? io->cache->Count(list) : -1;
    if (rec) io->cache->Begin(list);
    // epoch_shuffle=1: the part's rows in this epoch's order; -1: its ring no longer fits
    DeviceReshuffler* rs = train && n_cached >= 0 && io->resh && (*io->resh)[part]
                               ? (*io->resh)[part].get()
                               : nullptr;
    int64_t n_shuffled = -1;
    if (rs) {
      const double tb = Now();
      n_shuffled = rs->BeginEpoch(rs_epoch_key(P.shuffle_seed, (uint64_t)epoch, (uint64_t)list));
      io->shuffle_wait[0] += Now() - tb;
    }
    if (n_shuffled >= 0)
      StepReshuffled(&s, rs);
    else if (n_cached >= 0)
      StepReplayed(&s, list, n_cached);
    else if (io->feed)
      StepDeviceReader(&s, part, rec);
    else
      StepHostReader(&s, part, rec);
    if (rec) io->cache->Seal();
    const double tj = Now();
    const Progress p = learner->TakeProgress();
    io->step_s[1] += Now() - tj;
    prog.nrows += p.nrows;
    prog.loss += p.loss;
    prog.auc += p.auc;
  }
  if (s.fallback)
    std::printf("parse=device: %zu chunk%s parsed by the host (needs_host)\n", s.fallback,
                s.fallback == 1 ? "" : "s");
  return prog;
}

// ---- the sharded store ----------------------------------------------------------------------
// a batch in device memory, uploaded on the context's stream (three per shard in flight)
struct DevBatch {
  dfx_ctx* c = nullptr;
  std::unique_ptr<DevArray<uint64_t>> off, idx;
  std::unique_ptr<DevArray<float>> val, lab, wt;
  dfx_batch b{};
  void Upload(dfx_ctx* ctx, const RowBlockContainer<feaid_t>* blk) {
    if (!off) {
      c = ctx;
      off.reset(new DevArray<uint64_t>(c));
      idx.reset(new DevArray<uint64_t>(c));
      val.reset(new DevArray<float>(c));
      lab.reset(new DevArray<float>(c));
      wt.reset(new DevArray<float>(c));
    }
    const size_t B = blk ? blk->Size() : 0, nnz = blk ? blk->index.size() : 0;
    static const uint64_t zero = 0;
    b = dfx_batch{};
    b.size = (int64_t)B;
    b.nnz = (int64_t)nnz;
    b.offset = blk ? reinterpret_cast<uint64_t*>(off->upload(
                         reinterpret_cast<const uint64_t*>(blk->offset.data()), B + 1))
                   : off->upload(&zero, 1);
    b.index = nnz ? idx->upload(blk->index.data(), nnz) : nullptr;
    b.value = blk && !blk->value.empty() ? val->upload(blk->value.data(), nnz) : nullptr;
    b.label = B ? lab->upload(blk->label.data(), B) : nullptr;
    b.weight = blk && !blk->weight.empty() ? wt->upload(blk->weight.data(), B) : nullptr;
  }
};

std::string KwString(const KWArgs& kw) {
  std::string s;
  for (const auto& p : kw) {
    if (p.first == "fused") continue;
    if (!s.empty()) s += ",";
    s += p.first + "=" + p.second;
  }
  return s;
}

// What the sharded epoch needs of a store.  exchange=a2a: GpuShardedStore (KVStoreDist's
// exchanges, dist_host.h) over device batches; exchange=split: the owner-computes split behind
// GpuSplitLearner (split_learner.h), which takes host row blocks and device batches — one
// synchronous reference step per batch index on the concatenation of the shards' batches
// (push_agg=sum; pipelined=1 only overlaps model-free work, so the results equal the
// synchronous schedule).
class ShardRunner {
 public:
  /** local shard l's batch of a step: a host block (null: none, the shard gives an empty
   * batch), or batch `replay` of the cached list the step names */
  struct Item {
    const RowBlockContainer<feaid_t>* host = nullptr;
    int64_t replay = -1;
    // parse=auto-sharded: a batch the shard's DeviceBatchReader formed.  It holds a ring entry
    // or a text slot of `feed` until the runner marks `ticket`, which it does after the call
    // that queued the batch's last reader (see Mark below)
    const dfx_batch* dev = nullptr;
    DeviceTextFeed* feed = nullptr;
    uint64_t ticket = 0;
  };
  // A feed batch's mark.  Both stores read a worker's batch twice: at the submit that takes it
  // (a2a: the Localizer, dfx_dist_localize; split: dfx_split_partition), and in the step's main
  // part (a2a: dfx_dist_fwd_bwd reads offsets, values, labels; split: dfx_split_combine reads
  // the labels for the loss), which runs on the context stream — inside the same submit with
  // pipelined=0, inside the NEXT submit or the flush with pipelined=1.  Nothing later reads it
  // (the gradient push and the split's backward work on the step's own buffers).  So the
  // deferral is one Step call at most, the mark's event goes on the context stream, and a
  // sharded feed has kShardFeedDepth >= 1 + 2 ring entries and slots.
  struct Mark {
    DeviceTextFeed* feed;
    uint64_t ticket;
  };
  static void MarkAll(std::vector<Mark>* v) {
    for (const Mark& m : *v) m.feed->Mark(m.ticket);
    v->clear();
  }
  static constexpr int kShardFeedDepth = 4;
  virtual ~ShardRunner() {}
  virtual int nlocal() const = 0;
  virtual int nranks() const = 0;
  virtual int rank(int local) const = 0;
  virtual dfx_ctx* ctx(int local) const = 0;
  virtual const char* tag() const = 0;  // in the Training line, after the shard count
  virtual void AllReduceSum(std::vector<double>* v) = 0;
  /** one step of every local shard.  record: the host blocks are also appended to `list` of
   * the shards' caches.  preds (evaluation jobs): the step runs before the call returns and
   * preds[l] holds local shard l's predictions; without it the step may only be queued.
   * writers (with preds, pred_write=device): nothing comes down; local shard l's predictions
   * and device labels go to writers[l] instead and preds is left alone */
  virtual void Step(const std::vector<Item>& items, int64_t list, bool record, int job_type,
                    bool push_cnt, std::vector<std::vector<real_t>>* preds,
                    std::vector<std::unique_ptr<DevicePredWriter>>* writers = nullptr) = 0;
  /** run what is queued and apply the last push */
  virtual void Flush() = 0;
  /** host seconds the store made the submitting thread wait on its run-ahead bound */
  virtual double TakeThrottleSeconds() { return 0; }
  // the batch cache (cache=device, cache=auto): a sealed list's batches of local shard
  // l, -1 when the part has to be read; the recording pass's list brackets; the shards' sums
  bool has_cache() const { return !caches_.empty(); }
  int64_t Cached(int l, int64_t list) { return caches_[l]->Count(list); }
  void BeginList(int64_t list) {
    for (auto& c : caches_) c->Begin(list);
  }
  void SealList() {
    for (auto& c : caches_) c->Seal();
  }
  void CacheSums(std::vector<double>* cs) {
    cs->assign(4, 0.0);
    for (auto& c : caches_) {
      const DeviceBatchCache::Stats s = c->GetStats();
      (*cs)[0] += (double)s.batches;
      (*cs)[1] += (double)s.bytes;
      (*cs)[2] += (double)s.dropped;
      (*cs)[3] += (double)(s.sealed + s.dropped);
    }
  }

 protected:
  // each local shard's batch cache on its own context, recorded in the first epoch this run
  // executes.  A runner calls it once its contexts exist, and clears caches_ before they go.
  void MakeCaches(const RunPlan& plan, int64_t bytes) {
    for (int l = 0; plan.cache && l < nlocal(); ++l)
      caches_.emplace_back(new DeviceBatchCache(ctx(l), bytes));
  }
  std::vector<std::unique_ptr<DeviceBatchCache>> caches_;
};

class A2aRunner : public ShardRunner {
 public:
  A2aRunner(const Param& P, const KWArgs& rest, const LaunchEnv& env, const RunPlan& plan)
      : pipelined_(P.pipelined) {
    const int nlocal = plan.rccl ? 1 : P.shards;
    ctxs_.assign(nlocal, nullptr);
    const std::string kw = KwString(rest);
    for (int l = 0; l < nlocal; ++l)
      DfxCheck(dfx_ctx_create(plan.rccl ? env.local_rank : 0, kw.c_str(), &ctxs_[l]),
               "dfx_ctx_create");
    if (plan.rccl)
      ex_ = MakeRcclExchange(ctxs_[0], env.rank, env.world, env.comm_id_file);
    else
      ex_ = MakeLoopbackExchange(ctxs_);
    store_.reset(new GpuShardedStore(ex_.get(), P.pipelined));
    dev_.resize(nlocal);
    for (auto& v : dev_) v.resize(3);
    MakeCaches(plan, P.cache_mb << 20);
  }
  ~A2aRunner() override {
    store_.reset();  // flushes and joins the contexts
    dpred_.clear();
    caches_.clear();
    dev_.clear();
    ex_.reset();
    for (auto c : ctxs_) dfx_ctx_destroy(c);
  }
  int nlocal() const override { return ex_->nlocal(); }
  int nranks() const override { return ex_->nranks(); }
  int rank(int local) const override { return ex_->rank(local); }
  dfx_ctx* ctx(int local) const override { return ctxs_[local]; }
  const char* tag() const override { return ""; }
  void AllReduceSum(std::vector<double>* v) override { ex_->AllReduceSum(v); }
  void Step(const std::vector<Item>& items, int64_t list, bool record, int job_type,
            bool push_cnt, std::vector<std::vector<real_t>>* preds,
            std::vector<std::unique_ptr<DevicePredWriter>>* writers) override {
    const int L = nlocal();
    std::vector<dfx_batch> bs(L);
    std::vector<Mark> now;  // this step's feed batches
    for (int l = 0; l < L; ++l) {
      if (items[l].replay >= 0) {
        bs[l] = caches_[l]->Get(list, items[l].replay);
        continue;
      }
      if (items[l].dev) {  // as it is; the cache's copy runs on the feed's stream, behind the gathers
        bs[l] = *items[l].dev;
        if (record) caches_[l]->Append(bs[l]);
        now.push_back(Mark{items[l].feed, items[l].ticket});
        continue;
      }
      DevBatch& db = dev_[l][ring_];  // three per shard: a queued step still reads the last
      db.Upload(ctxs_[l], items[l].host);
      bs[l] = db.b;
      if (record && items[l].host) caches_[l]->Append(db.b);
    }
    ring_ = (ring_ + 1) % 3;
    if (!preds) {
      store_->Submit(bs, job_type, push_cnt);
      // pipelined: this Submit ran the step before, whose fwd_bwd was its batches' last reader;
      // else this step ran
      if (pipelined_) {
        MarkAll(&queued_marks_);
        queued_marks_.swap(now);
      } else {
        MarkAll(&now);
      }
      return;
    }
    // a submitted step runs at the next Submit or at Flush: flush, then its predictions come
    // down behind it on the contexts' streams
    if (dpred_.empty())
      for (int l = 0; l < L; ++l) dpred_.emplace_back(new DevArray<float>(ctxs_[l]));
    std::vector<float*> dp(L);
    for (int l = 0; l < L; ++l) {
      dpred_[l]->ensure((size_t)bs[l].size);
      dp[l] = dpred_[l]->get();
    }
    store_->Submit(bs, job_type, push_cnt, dp);
    store_->Flush();
    if (writers) {  // (a DevBatch is uploaded into again three steps on)
      for (int l = 0; l < L; ++l)
        if (bs[l].size) (*writers)[l]->Submit(bs[l].label, dp[l], bs[l].size);
    }
    // every step ran, and the writers' reads of the device labels are queued
    MarkAll(&queued_marks_);
    MarkAll(&now);
    if (writers) return;
    preds->resize(L);
    for (int l = 0; l < L; ++l) {
      (*preds)[l].resize((size_t)bs[l].size);
      dpred_[l]->download((*preds)[l].data(), (size_t)bs[l].size);
    }
  }
  void Flush() override {
    store_->Flush();
    MarkAll(&queued_marks_);  // the queued step ran
  }

 private:
  const bool pipelined_;
  std::vector<Mark> queued_marks_;  // the queued step's feed batches (pipelined)
  std::vector<dfx_ctx*> ctxs_;
  std::unique_ptr<ShardExchange> ex_;
  std::unique_ptr<GpuShardedStore> store_;
  std::vector<std::vector<DevBatch>> dev_;
  std::vector<std::unique_ptr<DevArray<float>>> dpred_;
  int ring_ = 0;
};

class SplitRunner : public ShardRunner {
 public:
  SplitRunner(const Param& P, const KWArgs& rest, const RunPlan& plan) {
    KWArgs kw = rest;
    kw.push_back({"pipelined", P.pipelined ? "1" : "0"});
    sl_ = plan.rccl ? GpuSplitLearner::CreateRccl(kw)
                    : GpuSplitLearner::CreateLoopback(P.shards, kw);
    MakeCaches(plan, P.cache_mb << 20);
  }
  ~SplitRunner() override {
    // no queued step reads a cached batch any more; the caches go before the contexts, which
    // are the learner's
    try {
      sl_->Sync();
    } catch (...) {
    }
    caches_.clear();
    sl_.reset();
  }
  int nlocal() const override { return sl_->nlocal(); }
  int nranks() const override { return sl_->nranks(); }
  int rank(int local) const override { return sl_->rank(local); }
  dfx_ctx* ctx(int local) const override { return sl_->shard(local); }
  const char* tag() const override { return ", split"; }
  void AllReduceSum(std::vector<double>* v) override { sl_->AllReduceSum(v); }
  void Step(const std::vector<Item>& items, int64_t list, bool record, int job_type,
            bool push_cnt, std::vector<std::vector<real_t>>* preds,
            std::vector<std::unique_ptr<DevicePredWriter>>* writers) override {
    const int L = nlocal();
    std::vector<dmlc::RowBlock<feaid_t>> blk(L);
    std::vector<dfx_batch> dev(L);
    std::vector<GpuSplitLearner::Item> it(L);
    std::vector<Mark> now;  // feed batches this call marks itself
    for (int l = 0; l < L; ++l) {
      if (items[l].replay >= 0) {
        dev[l] = caches_[l]->Get(list, items[l].replay);
        it[l].dev = &dev[l];
      } else if (items[l].dev) {
        // a feed's batch, as it is.  The learner makes no feeder while no host item is pending
        // (Impl::Feeders), and a run with feeds gives it none, so the context's input stream
        // stays the feed's.  The learner calls the release hook after the submit that queued
        // the batch's combine; with a writer the step runs inside the call and the mark waits
        // for the writer's read of the labels instead (below).
        dev[l] = *items[l].dev;
        it[l].dev = &dev[l];
        DeviceTextFeed* const feed = items[l].feed;
        const uint64_t ticket = items[l].ticket;
        if (preds && writers)
          now.push_back(Mark{feed, ticket});
        else
          it[l].release = [feed, ticket]() { feed->Mark(ticket); };
        // recorded on the feed's stream, behind the gathers and before the partition's wait
        if (record && !caches_.empty()) caches_[l]->Append(dev[l]);
      } else if (items[l].host) {
        blk[l] = items[l].host->GetBlock();
        it[l].host = &blk[l];
      }  // else none: the shard gives an empty batch
    }
    const bool rec = record && !caches_.empty();
    std::vector<dfx_batch> up;
    if (preds && writers) {  // (a staging slot is uploaded into again three steps on)
      std::vector<const float*> dp;
      sl_->ProcessDeviceBatches(it, job_type, push_cnt, nullptr, &up, &dp);
      for (int l = 0; l < L; ++l)
        if (up[l].size) (*writers)[l]->Submit(up[l].label, dp[l], up[l].size);
      MarkAll(&now);
      return;
    }
    sl_->ProcessDeviceBatches(it, job_type, push_cnt, preds, rec ? &up : nullptr);
    // the copies run on the contexts' input streams, behind the uploads and before the staging
    // slots are reused (as the single-GPU path's, RunEpoch)
    for (int l = 0; rec && l < L; ++l)
      if (items[l].host) caches_[l]->Append(up[l]);
  }
  void Flush() override { sl_->Flush(); }
  double TakeThrottleSeconds() override { return sl_->TakeThrottleSeconds(); }

 private:
  std::shared_ptr<GpuSplitLearner> sl_;
};

// a part's batches: training reads minibatches (sgd_learner.cc:273-280), validation and
// prediction whole 256 MB chunks, one batch per chunk, never shuffled or down-sampled
// (sgd_learner.cc:281-286)
class PartReader {
 public:
  PartReader(const Param& P, bool train, int part, int nparts) {
    if (train)
      batches_.reset(new ThreadedBatchReader(P.data_in, P.data_format, part, nparts, P.batch_size,
                                             P.batch_size * P.shuffle, P.neg_sampling,
                                             P.nthreads));
    else
      chunks_.reset(new TextReader(P.data_val, P.data_format, part, nparts, 256 << 20,
                                   P.nthreads));
  }
  bool Next() {
    if (batches_) return batches_->Next();
    while (chunks_->Next())
      if (chunks_->Value().Size() != 0) return true;
    return false;
  }
  const RowBlockContainer<feaid_t>& Value() const {
    return batches_ ? batches_->Value() : chunks_->Value();
  }

 private:
  std::unique_ptr<ThreadedBatchReader> batches_;
  std::unique_ptr<TextReader> chunks_;
};

// One pass of one job kind over the shards' parts, the one epoch loop of both exchanges: for
// job j the shard of global rank g reads part j * nshards + g of num_jobs_per_epoch * nshards
// (or replays the batches it cached for it), the shards step together (an exhausted shard
// gives empty batches until the all-reduced "any shard still has a batch" is 0), then the
// store is flushed and the progress summed over every shard of every rank.
struct ShardIO {  // what a pass may use (null: not in this run) and what it reports (accumulated)
  // prediction: local shard l's rows go to (*pred_files)[l] in the order read, through
  // (*writers)[l] with pred_write=device
  const std::vector<FILE*>* pred_files = nullptr;
  std::vector<std::unique_ptr<DevicePredWriter>>* writers = nullptr;
  // parse=auto-sharded: local shard l's parts are read by a DeviceBatchReader on (*feeds)[l]
  // instead of a PartReader: the same parts, chunks and batches, formed on the device.  A
  // reader lives for one job; the batches it handed out may be marked after it is gone (the
  // feed keeps that state).
  std::vector<std::unique_ptr<DeviceTextFeed>>* feeds = nullptr;
  double host_s[2] = {0, 0};  // host seconds inside Step; inside the per-step all-reduce
  DeviceBatchReader::Times times;  // the device readers'
};
Progress ShardedPass(ShardRunner* run, const Param& P, int epoch, int job_type, bool record,
                     ShardIO* io) {
  const std::vector<FILE*>* const pred_files = io->pred_files;
  const auto writers = io->writers;
  const auto feeds = io->feeds;
  const int nlocal = run->nlocal(), nshards = run->nranks();
  const bool train = job_type == GpuSGDLearner::kTraining;
  const int nparts = P.num_jobs_per_epoch * nshards;
  std::vector<std::vector<real_t>> preds;
  double fallback = 0;
  for (int job = 0; job < P.num_jobs_per_epoch; ++job) {
    const int64_t list = CacheList(P, train, job);
    const bool rec = record && run->has_cache();
    std::vector<std::unique_ptr<PartReader>> rd(nlocal);
    std::vector<std::unique_ptr<DeviceBatchReader>> drd(nlocal);
    std::vector<int64_t> n_cached(nlocal, -1), pos(nlocal, 0);
    for (int l = 0; l < nlocal; ++l) {
      if (run->has_cache() && !record) n_cached[l] = run->Cached(l, list);
      if (n_cached[l] >= 0) continue;
      const int part = job * nshards + run->rank(l);
      if (feeds)
        drd[l] = MakeDeviceReader(P, (*feeds)[l].get(), train, part, nparts);
      else
        rd[l].reset(new PartReader(P, train, part, nparts));
    }
    if (rec) run->BeginList(list);
    std::vector<bool> more(nlocal, true);
    for (;;) {
      std::vector<double> any(1, 0.0);
      for (int l = 0; l < nlocal; ++l) {
        if (more[l])
          more[l] = drd[l] ? drd[l]->Next() : rd[l] ? rd[l]->Next() : pos[l] < n_cached[l];
        if (more[l]) any[0] += 1;
      }
      const double ta = Now();
      run->AllReduceSum(&any);
      io->host_s[1] += Now() - ta;
      if (any[0] == 0) break;
      std::vector<ShardRunner::Item> items(nlocal);
      for (int l = 0; l < nlocal; ++l) {
        if (!more[l]) continue;
        if (drd[l]) {
          items[l].dev = &drd[l]->Value();
          items[l].feed = (*feeds)[l].get();
          items[l].ticket = drd[l]->Ticket();
        } else if (rd[l]) {
          items[l].host = &rd[l]->Value();
        } else {
          items[l].replay = pos[l]++;
        }
      }
      const double ts = Now();
      run->Step(items, list, rec, job_type, train && epoch == 0, pred_files ? &preds : nullptr,
                pred_files ? writers : nullptr);
      io->host_s[0] += Now() - ts;
      for (int l = 0; pred_files && !writers && l < nlocal; ++l) {
        if (!items[l].host && !items[l].dev) continue;
        // (a feed's batch: the chunk's labels as the parse copied them back, until the next Next)
        WritePredRows((*pred_files)[l],
                      items[l].dev ? drd[l]->HostLabels() : items[l].host->label.data(),
                      preds[l].data(), preds[l].size(), P.pred_prob);
      }
    }
    if (rec) run->SealList();
    for (int l = 0; l < nlocal; ++l) {
      if (!drd[l]) continue;
      fallback += (double)drd[l]->FallbackChunks();
      io->times += drd[l]->TimesSpent();
    }
  }
  run->Flush();
  if (writers)
    for (auto& w : *writers) w->Finish();
  if (feeds) {  // every rank calls: the chunks the device handed back, over shards and ranks
    std::vector<double> fb(1, fallback);
    run->AllReduceSum(&fb);
    if (fb[0] > 0 && run->rank(0) == 0)
      std::printf("parse=device: %.0f chunk%s parsed by the host (needs_host)\n", fb[0],
                  fb[0] == 1 ? "" : "s");
  }
  std::vector<double> pr(3, 0.0);
  for (int l = 0; l < nlocal; ++l) {
    dfx_progress p;
    DfxCheck(dfx_progress_read(run->ctx(l), &p, 1), "dfx_progress_read");
    pr[0] += p.nrows;
    pr[1] += p.loss;
    pr[2] += p.auc;
  }
  run->AllReduceSum(&pr);
  Progress out;
  out.nrows = pr[0];
  out.loss = pr[1];
  out.auc = pr[2];
  return out;
}

// the sharded runs: training (with data_val: a validation pass after every epoch) and task=2
int RunSharded(const Param& P, const KWArgs& rest, const LaunchEnv& env, const RunPlan& plan) {
  std::unique_ptr<ShardRunner> run;
  if (P.exchange == "split")
    run.reset(new SplitRunner(P, rest, plan));
  else
    run.reset(new A2aRunner(P, rest, env, plan));
  const int nlocal = run->nlocal(), nshards = run->nranks(), rank = run->rank(0);
  if (!P.model_in.empty()) {
    const int it = P.load_epoch > 0 ? P.load_epoch : -1;
    for (int l = 0; l < nlocal; ++l) {
      if (P.model_in_parts <= 0 || P.model_in_parts == nshards) {
        DfxCheck(dfx_store_load(run->ctx(l), ModelNamePart(P.model_in, it, run->rank(l)).c_str()),
                 "dfx_store_load");
      } else {  // saved by a different number of servers: keep the keys this shard owns
        for (int r = 0; r < P.model_in_parts; ++r)
          DfxCheck(dfx_store_load_part(run->ctx(l), ModelNamePart(P.model_in, it, r).c_str(),
                                       run->rank(l), nshards),
                   "dfx_store_load_part");
      }
    }
  }
  // parse=auto-sharded: one text feed per local shard on the shard's context, for the whole run.
  // Its loader stream is the context's input stream while it lives.  The feeds go before the
  // runner, which owns the contexts, and after a flush: a queued step reads a feed's batch and
  // its mark calls into the feed.
  struct Feeds {
    ShardRunner* run;
    std::vector<std::unique_ptr<DeviceTextFeed>> v;
    ~Feeds() {
      if (v.empty()) return;
      try {
        run->Flush();
      } catch (...) {
      }
      v.clear();
    }
  } feeds{run.get(), {}};
  if (plan.parse == RunPlan::Parse::kDevice)
    for (int l = 0; l < nlocal; ++l)
      feeds.v.emplace_back(new DeviceTextFeed(run->ctx(l), P.batch_size, P.batch_size * P.shuffle,
                                              P.data_format, ShardRunner::kShardFeedDepth,
                                              ShardRunner::kShardFeedDepth));
  std::vector<std::unique_ptr<DeviceTextFeed>>* const fp = feeds.v.empty() ? nullptr : &feeds.v;
  const int kfirst = std::max(0, P.load_epoch > 0 ? P.load_epoch + 1 : 0);
  if (P.task == 2) {  // one pass over data_val; every worker saves its own rows (SavePred)
    std::vector<FILE*> files;
    if (!P.pred_out.empty()) {
      for (int l = 0; l < nlocal; ++l) {
        const std::string name = P.pred_out + "_part-" + std::to_string(run->rank(l));
        files.push_back(std::fopen(name.c_str(), "w"));
        if (!files.back()) {
          std::fprintf(stderr, "cannot open %s\n", name.c_str());
          for (FILE* f : files)
            if (f) std::fclose(f);
          return 1;
        }
      }
    }
    // pred_write=device: one writer per local shard, on the shard's context (they go before
    // the runner, which owns the contexts)
    std::vector<std::unique_ptr<DevicePredWriter>> writers;
    if (plan.pred_write_device)
      for (size_t l = 0; l < files.size(); ++l)
        writers.emplace_back(new DevicePredWriter(run->ctx((int)l), files[l], P.pred_prob));
    ShardIO io;
    io.pred_files = files.empty() ? nullptr : &files;
    io.writers = writers.empty() ? nullptr : &writers;
    io.feeds = fp;
    const double tp = Now();
    const Progress pr = ShardedPass(run.get(), P, kfirst, GpuSGDLearner::kPrediction, false, &io);
    const double pass_s = Now() - tp;
    for (FILE* f : files) std::fclose(f);
    if (rank == 0) std::printf("Prediction: %s\n", Text(pr).c_str());
    if (plan.pred_write_device) {
      DevicePredWriter::Stats sum;
      for (auto& w : writers) sum += w->GetStats();
      PrintPredWriteLine(sum, pass_s);
    }
    writers.clear();
    return 0;
  }
  const double t0 = Now();
  double pre_loss = 0, pre_val_auc = 0;
  for (int k = kfirst; k < P.max_num_epochs; ++k) {
    const double te = Now();
    const bool record = k == kfirst;  // the first epoch this run executes records
    // exchange=split with the cache: where the submitting thread's time went
    const bool timed = run->has_cache() && P.exchange == "split";
    if (timed) (void)run->TakeThrottleSeconds();
    ShardIO io;
    io.feeds = fp;
    const Progress tr = ShardedPass(run.get(), P, k, GpuSGDLearner::kTraining, record, &io);
    const double dt = Now() - te;
    const DeviceBatchReader::Times& rt = io.times;
    if (rank == 0)
      std::printf("Epoch[%d] Training: %s  (%.0f ex/s incl. parse+PCIe, %d shards%s, %.2f s)\n", k,
                  Text(tr).c_str(), tr.nrows / dt, nshards, run->tag(), Now() - t0);
    if (timed && rank == 0)
      std::printf("  split: epoch %.3f s; the host spent %.3f s in Step (of it %.3f s waiting on "
                  "the store's run-ahead bound) and %.3f s in the per-step all-reduce\n",
                  dt, io.host_s[0], run->TakeThrottleSeconds(), io.host_s[1]);
    // where this process's device readers' time went, summed over its shards (Times); an
    // epoch that replayed every part from the cache made no reader and prints nothing
    if (fp && rank == 0 && rt.copy + rt.wait_text + rt.wait_parse + rt.wait_step > 0)
      std::printf("  reader: epoch %.3f s, host copy %.3f s (loader threads); the caller waited "
                  "for text %.3f s, for the parse %.3f s, for a ring batch %.3f s\n",
                  dt, rt.copy, rt.wait_text, rt.wait_parse, rt.wait_step);
    Progress va;
    if (!P.data_val.empty()) {
      // (the pass above flushed: the 1-step-stale schedule's last push is applied)
      const double tv = Now();
      ShardIO vio;
      vio.feeds = fp;
      va = ShardedPass(run.get(), P, k, GpuSGDLearner::kValidation, record, &vio);
      if (rank == 0)
        std::printf("Epoch[%d] Validation: %s  (%.0f ex/s)\n", k, Text(va).c_str(),
                    va.nrows / (Now() - tv));
    }
    if (record && run->has_cache()) {  // rank 0 prints the shards' sums
      std::vector<double> cs;
      run->CacheSums(&cs);
      run->AllReduceSum(&cs);
      if (rank == 0) PrintCacheLine(cs[0], cs[1], cs[2], cs[3]);
    }
    std::fflush(stdout);
    // on the all-reduced sums: the same on every rank, so all of them leave the loop in the
    // same epoch
    if (ShouldStop(tr, va, &pre_loss, &pre_val_auc, P, false)) break;
  }
  run->Flush();
  if (!P.model_out.empty()) {
    ModelWriteStats sum;  // model_write=device: this process's shards
    sum.entries = 0;
    const double t0 = Now();
    for (int l = 0; l < nlocal; ++l) {
      const std::string name = ModelNamePart(P.model_out, -1, run->rank(l));
      DfxCheck(dfx_sync(run->ctx(l)), "dfx_sync");
      if (plan.model_write_device) {
        int64_t st[4];
        double tm[2];
        DfxCheck(dfx_store_save_dev(run->ctx(l), name.c_str(), P.has_aux ? 1 : 0, 0, st, tm),
                 "dfx_store_save_dev");
        sum.entries += st[0];
        sum.bytes += st[1];
        sum.wait_s += tm[0];
      } else {
        DfxCheck(dfx_store_save(run->ctx(l), name.c_str(), P.has_aux ? 1 : 0), "dfx_store_save");
      }
    }
    if (plan.model_write_device) PrintModelWriteLine(sum, Now() - t0);
  }
  return 0;
}

// task=1 (src/main.cc:81-87 with src/reader/dump.h): model_in, the literal file (dump.h:55-56
// opens it as it is named), into name_dump as SGDUpdater::Dump's text
int RunDump(const Param& P, KWArgs rest, const RunPlan& plan) {
  if (!plan.fused_given) rest.push_back({"fused", "1"});
  GpuSGDLearner learner(rest);  // (the context and its updater; nothing is trained)
  DfxCheck(dfx_store_load(learner.context(), P.model_in.c_str()), "dfx_store_load");
  const ModelWriteStats st = learner.updater()->DumpFile(P.name_dump, P.dump_aux, P.need_reverse,
                                                         plan.model_write_device);
  std::printf("Dump: %lld entries, %lld bytes in %.3f s\n", (long long)st.entries,
              (long long)st.bytes, st.seconds);
  if (plan.model_write_device && st.host_chunks)
    std::printf("model_write=device: %lld of %lld chunk%s written by the host (a float outside "
                "the device formatter's domain)\n",
                (long long)st.host_chunks, (long long)st.chunks, st.chunks == 1 ? "" : "s");
  return 0;
}

// the single-GPU runs: training (with data_val: a validation pass after every epoch) and task=2
int RunSingle(const Param& P, KWArgs rest, const RunPlan& plan) {
  if (!plan.fused_given) rest.push_back({"fused", "1"});
  GpuSGDLearner learner(rest);
  std::unique_ptr<DeviceTextFeed> feed;
  if (plan.parse == RunPlan::Parse::kDevice)
    feed.reset(new DeviceTextFeed(learner.context(), P.batch_size, P.batch_size * P.shuffle,
                                  P.data_format));
  // (declared after the learner and the feed: destroyed, joining the context, before them)
  std::unique_ptr<DeviceBatchCache> cache;
  if (plan.cache) cache.reset(new DeviceBatchCache(learner.context(), P.cache_mb << 20));
  // epoch_shuffle=1: one reshuffler per training part, made after the recording epoch (declared
  // after the cache: destroyed before it)
  std::vector<std::unique_ptr<DeviceReshuffler>> resh;
  int k0 = 0;
  if (!P.model_in.empty()) {  // sgd_learner.cc:58-67
    FileStream fi(ModelName(P.model_in, P.load_epoch > 0 ? P.load_epoch : -1).c_str(), "rb");
    learner.updater()->Load(&fi);
    if (P.load_epoch > 0) k0 = P.load_epoch + 1;
  }
  if (P.task == 2) {  // prediction, sgd_learner.cc:69-77
    FILE* pf = nullptr;
    if (!P.pred_out.empty()) {
      pf = std::fopen((P.pred_out + "_part-0").c_str(), "w");
      if (!pf) {
        std::fprintf(stderr, "cannot open %s_part-0\n", P.pred_out.c_str());
        return 1;
      }
    }
    std::unique_ptr<DevicePredWriter> writer;
    if (pf && plan.pred_write_device)
      writer.reset(new DevicePredWriter(learner.context(), pf, P.pred_prob));
    PassIO io;
    io.feed = feed.get();
    io.pred_file = pf;
    io.dev_writer = writer.get();
    const double tp = Now();
    const Progress pr = RunEpoch(&learner, P, plan, k0, GpuSGDLearner::kPrediction, &io);
    if (writer) writer->Finish();
    const double pass_s = Now() - tp;
    if (pf) std::fclose(pf);
    std::printf("Prediction: %s\n", Text(pr).c_str());
    if (plan.pred_write_device)
      PrintPredWriteLine(writer ? writer->GetStats() : DevicePredWriter::Stats(), pass_s);
    writer.reset();
    return 0;
  }
  const double t0 = Now();
  double pre_loss = 0, pre_val_auc = 0;  // sgd_learner.cc:52
  for (int k = k0; k < P.max_num_epochs; ++k) {
    const double te = Now();
    const bool record = k == k0;  // the first epoch this run executes records
    PassIO io;
    io.feed = feed.get();
    io.cache = cache.get();
    io.record = record;
    // (epoch_resample=1 makes a part's reshuffler inside the recording epoch)
    if (plan.epoch_resample && resh.empty()) resh.resize((size_t)P.num_jobs_per_epoch);
    io.resh = resh.empty() ? nullptr : &resh;
    const Progress tr = RunEpoch(&learner, P, plan, k, GpuSGDLearner::kTraining, &io);
    const double dt = Now() - te;
    std::printf("Epoch[%d] Training: %s  (%.0f ex/s incl. parse+PCIe, %.2f s)\n", k,
                Text(tr).c_str(), tr.nrows / dt, Now() - t0);
    if (plan.epoch_resample) {
      std::printf("  epoch_resample: %lld of %lld rows kept in %.0f parts",
                  (long long)io.resample_rows[0], (long long)io.resample_rows[1],
                  io.shuffle_wait[1]);
      if (io.resample_read)
        std::printf(", %d part%s read through %s", io.resample_read,
                    io.resample_read == 1 ? "" : "s",
                    io.resample_read == 1 ? "its reader" : "their readers");
      std::printf("\n");
    }
    if (io.shuffle_wait[1] > 0)
      std::printf("  epoch_shuffle: %.0f parts reshuffled, the host waited %.3f ms for their "
                  "batches' sizes\n",
                  io.shuffle_wait[1], io.shuffle_wait[0] * 1e3);
    if (feed)  // where the device reader's time went (device_reader.h Times)
      std::printf("  reader: epoch %.3f s, host copy %.3f s (loader thread); caller waited for "
                  "text %.3f s, for the parse %.3f s, for a ring batch %.3f s, in dfx_train_step "
                  "%.3f s, in the final join %.3f s\n",
                  dt, io.times.copy, io.times.wait_text, io.times.wait_parse, io.times.wait_step,
                  io.step_s[0], io.step_s[1]);
    Progress va;
    if (!P.data_val.empty()) {
      PassIO vio;
      vio.feed = feed.get();
      vio.cache = cache.get();
      vio.record = record;
      va = RunEpoch(&learner, P, plan, k, GpuSGDLearner::kValidation, &vio);
      std::printf("Epoch[%d] Validation: %s\n", k, Text(va).c_str());
    }
    if (cache && record) {
      const DeviceBatchCache::Stats cs = cache->GetStats();
      PrintCacheLine((double)cs.batches, (double)cs.bytes, (double)cs.dropped,
                     (double)(cs.sealed + cs.dropped));
      if (plan.cache_loc) {
        const DeviceBatchCache::LocStats ls = cache->GetLocStats();
        // (held counts whole blocks; the outputs' own bytes, each array rounded to 256)
        std::printf("cache_loc=1: %lld of %lld batches hold Localizer outputs, %.1f MB of the "
                    "%.1f MB held\n",
                    (long long)ls.batches, (long long)cs.batches, (double)ls.bytes / (1 << 20),
                    (double)cs.bytes / (1 << 20));
      }
      if (plan.epoch_shuffle) {
        int made = 0;
        int64_t ring = 0, scratch = 0;
        resh.resize((size_t)P.num_jobs_per_epoch);
        for (int part = 0; part < P.num_jobs_per_epoch; ++part) {
          const int64_t list = CacheList(P, true, part);
          if (plan.epoch_resample) {  // made, or found not to fit, while the part was recorded
            if (!resh[part]) continue;
          } else {
            if (cache->Count(list) < 0) continue;  // not cached: read as without the option
            resh[part].reset(new DeviceReshuffler(cache.get(), list, (int64_t)P.batch_size, 4));
            if (!resh[part]->kept()) {
              resh[part].reset();
              continue;
            }
          }
          const DeviceReshuffler::Stats rs = resh[part]->GetStats();
          ring += rs.ring_bytes;
          scratch += rs.scratch_bytes;
          ++made;
        }
        std::printf("epoch_shuffle=1: %d of %d training parts reshuffle, rings %.1f MB, scratch "
                    "%.1f MB\n",
                    made, P.num_jobs_per_epoch, (double)ring / (1 << 20),
                    (double)scratch / (1 << 20));
        if (plan.epoch_resample) {
          std::printf("epoch_resample=1: %d of %d training parts resample (neg_sampling=%g, every "
                      "epoch a fresh sample of the rows held)",
                      made, P.num_jobs_per_epoch, (double)P.neg_sampling);
          if (made < P.num_jobs_per_epoch)
            std::printf(", %d read through %s with the reader's sample",
                        P.num_jobs_per_epoch - made,
                        P.num_jobs_per_epoch - made == 1 ? "its reader" : "their readers");
          std::printf("\n");
        }
      }
    }
    std::fflush(stdout);
    if (ShouldStop(tr, va, &pre_loss, &pre_val_auc, P, true)) break;
  }
  if (!P.model_out.empty() && plan.model_write_device) {
    // the same file with no Stream, temporary file or copy of it between (either fused value:
    // the updater's own context holds the model)
    const ModelWriteStats st =
        learner.updater()->SaveFile(ModelName(P.model_out, -1), P.has_aux, true);
    PrintModelWriteLine(st, st.seconds);
  } else if (!P.model_out.empty()) {  // sgd_learner.cc:116-120
    FileStream fo(ModelName(P.model_out, -1).c_str(), "wb");
    learner.updater()->Save(P.has_aux, &fo);
  }
  return 0;
}
}  // namespace

// parse argv, resolve the options (train_options.h: every rule and line), say what was
// resolved, refuse or run
int main(int argc, char** argv) {
  Param P;
  KWArgs rest;
  RunPlan plan;
  std::vector<std::string> lines;
  std::string err;
  const LaunchEnv env = LaunchEnv::FromEnvironment();
  int rc = ParseArgs(argc, argv, &P, &rest, &err);
  if (rc == 0) rc = ResolveOptions(P, rest, env, &plan, &lines, &err);
  for (const std::string& line : lines) std::printf("%s\n", line.c_str());
  std::fflush(stdout);
  if (rc != 0) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  if (plan.dump) return RunDump(P, rest, plan);
  return plan.sharded ? RunSharded(P, rest, env, plan) : RunSingle(P, rest, plan);
}
