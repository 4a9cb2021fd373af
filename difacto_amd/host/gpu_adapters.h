// gpu_adapters.h — the reference's Localizer / Loss / Updater / Store implemented over
// libdifacto_amd.so's C-ABI (include/difacto_amd.h).  Host code only (no HIP headers):
// every device buffer is allocated, copied and freed through the C-ABI.
//
// These are the drop-in classes a maintainer registers in the reference's factories
// (INTEGRATION.md):
//   GpuLocalizer   src/data/localizer.h:16-95        Compact(blk, compacted, uniq, cnt)
//   GpuFMLoss      src/loss/fm_loss.h:29-213          loss=fm (V_dim > 0) / logit (V_dim 0)
//   GpuSGDUpdater  src/sgd/sgd_updater.h:74-180       the model lives in HBM
//   StoreGPU       src/store/store_local.h:17-59      inline Push/Pull into the updater
//   GpuSGDLearner  src/sgd/sgd_learner.cc:201-317     IterateData's per-batch executor, either
//                  through the interfaces above (Localizer -> Pull -> Predict -> Evaluate ->
//                  AUC -> CalcGrad -> Push) or as one fused dfx_train_step
//
// Inputs are host arrays (the reference's SArray / RowBlock); the adapters copy them to the
// device and back, so their rate is PCIe-inclusive.  The fused learner keeps the model and
// every intermediate in HBM and copies only the batch in.
#ifndef DIFACTO_AMD_HOST_GPU_ADAPTERS_H_
#define DIFACTO_AMD_HOST_GPU_ADAPTERS_H_

#include <cstdio>
#include <limits>

#include "../../include/difacto_amd.h"
#include "iface.h"

namespace difacto {

/** abort with dfx_last_error() on a non-zero status (the reference's LOG(FATAL)) */
void DfxCheck(int status, const char* what);

/** one device context (stream + workspace + device store), shared by the adapters */
class GpuContext {
 public:
  GpuContext(int device, const KWArgs& kwargs);
  ~GpuContext();
  dfx_ctx* h() const { return h_; }
  int V_dim() const { return dfx_ctx_vdim(h_); }

 private:
  dfx_ctx* h_ = nullptr;
};

/** a device array of T, grow-only */
template <typename T>
class DevArray {
 public:
  explicit DevArray(dfx_ctx* c) : c_(c) {}
  ~DevArray() {
    if (p_) dfx_free(c_, p_);
  }
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  T* get() const { return static_cast<T*>(p_); }
  void ensure(size_t n) {
    if (n <= cap_ && p_) return;
    if (p_) DfxCheck(dfx_free(c_, p_), "dfx_free");
    p_ = nullptr;
    DfxCheck(dfx_malloc(c_, &p_, (n ? n : 1) * sizeof(T)), "dfx_malloc");
    cap_ = n;
  }
  /** host -> device (n elements); returns the device pointer, or NULL when src is NULL */
  T* upload(const T* src, size_t n) {
    if (!src) return nullptr;
    ensure(n);
    if (n) DfxCheck(dfx_memcpy(c_, p_, src, n * sizeof(T), 0), "upload");
    return get();
  }
  void download(T* dst, size_t n) const {
    if (n) DfxCheck(dfx_memcpy(c_, dst, p_, n * sizeof(T), 1), "download");
    DfxCheck(dfx_sync(c_), "sync");
  }

 private:
  dfx_ctx* c_;
  void* p_ = nullptr;
  size_t cap_ = 0;
};

/** Localizer::Compact on the device (bit-exact with localizer.cc:11-107) */
class GpuLocalizer {
 public:
  explicit GpuLocalizer(std::shared_ptr<GpuContext> ctx,
                        feaid_t max_index = std::numeric_limits<feaid_t>::max())
      : ctx_(ctx), max_index_(max_index) {}
  void Compact(const dmlc::RowBlock<feaid_t>& blk, RowBlockContainer<unsigned>* compacted,
               std::vector<feaid_t>* uniq_idx = nullptr, std::vector<real_t>* idx_frq = nullptr);

 private:
  std::shared_ptr<GpuContext> ctx_;
  feaid_t max_index_;
};

/** FMLoss (fm_loss.h) / LogitLoss (logit_loss.h, == V_dim 0) on the device (kwarg `device`) */
class GpuFMLoss : public Loss {
 public:
  explicit GpuFMLoss(bool logit = false) : logit_(logit) {}
  KWArgs Init(const KWArgs& kwargs) override;
  /** param = {weights, w_pos, V_pos}; pred accumulates (+=) like the reference */
  void Predict(const dmlc::RowBlock<unsigned>& data, const std::vector<SArray<char>>& param,
               SArray<real_t>* pred) override;
  real_t Evaluate(dmlc::real_t const* label, const SArray<real_t>& pred) const override;
  /** param = {weights, w_pos, V_pos, pred}; grad accumulates (the caller zero-fills it) */
  void CalcGrad(const dmlc::RowBlock<unsigned>& data, const std::vector<SArray<char>>& param,
                SArray<real_t>* grad) override;
  /** BinClassMetric::AUC (bin_class_metric.h:35-57): AUC * n */
  real_t AUC(dmlc::real_t const* label, const SArray<real_t>& pred) const;
  int V_dim() const { return V_dim_; }

 private:
  struct Dev;
  void Upload(const dmlc::RowBlock<unsigned>& data, const std::vector<SArray<char>>& param);
  bool logit_;
  int V_dim_ = 0;
  std::shared_ptr<GpuContext> ctx_;
  std::shared_ptr<Dev> dev_;
};

/** what SaveFile / DumpFile wrote.  The device writers count everything; the host writers give
 * the file's bytes (its size), DumpFile its lines too (SaveFile: entries = -1, not counted).
 * seconds: the writer's call alone, not the counting */
struct ModelWriteStats {
  int64_t entries = -1, bytes = 0, chunks = 0, host_chunks = 0;
  double wait_s = 0, write_s = 0;  // host seconds waiting for a chunk, and writing
  double seconds = 0;
};

/** SGDUpdater (FTRL w, AdaGrad V, V_threshold InitV) with its model in HBM */
class GpuSGDUpdater : public Updater {
 public:
  GpuSGDUpdater() {}
  KWArgs Init(const KWArgs& kwargs) override;
  void Load(Stream* fi) override;
  void Save(bool save_aux, Stream* fo) const override;
  void Dump(bool dump_aux, bool need_reverse, Stream* fo) const override;
  /** Save and Dump straight to a path, with no Stream and no temporary file between: by the
   * device writers (dfx_store_save_dev / dfx_store_dump_dev) or, device = false, by the host
   * writers (dfx_store_save / dfx_store_dump).  The same bytes either way. */
  ModelWriteStats SaveFile(const std::string& path, bool save_aux, bool device) const;
  ModelWriteStats DumpFile(const std::string& path, bool dump_aux, bool need_reverse,
                           bool device) const;
  void Get(const SArray<feaid_t>& fea_ids, int data_type, SArray<real_t>* data,
           SArray<int>* data_offset) override;
  void Update(const SArray<feaid_t>& fea_ids, int data_type, const SArray<real_t>& data,
              const SArray<int>& data_offset) override;
  std::string Get_report() override;
  /** SGDUpdater::Evaluate (sgd_updater.cc:12-30): penalty and nnz(w) */
  void Evaluate(double* penalty, int64_t* nnz_w) const;
  std::shared_ptr<GpuContext> context() const { return ctx_; }
  int V_dim() const { return V_dim_; }

 private:
  void CopyThroughFile(bool save, bool aux, bool reverse, Stream* s) const;
  std::shared_ptr<GpuContext> ctx_;
  int V_dim_ = 0;
  double last_new_w_ = 0;
};

/** StoreLocal semantics (store_local.h:24-45): synchronous, callback inline */
class StoreGPU : public Store {
 public:
  KWArgs Init(const KWArgs& kwargs) override { return kwargs; }
  int Push(const SArray<feaid_t>& fea_ids, int val_type, const SArray<real_t>& vals,
           const SArray<int>& lens, const std::function<void()>& on_complete = nullptr) override;
  int Pull(const SArray<feaid_t>& fea_ids, int val_type, SArray<real_t>* vals, SArray<int>* lens,
           const std::function<void()>& on_complete = nullptr) override;
  void Wait(int time) override { (void)time; }
  int NumWorkers() override { return 1; }
  int NumServers() override { return 1; }
  int Rank() override { return 0; }

 private:
  int time_ = 0;
};

/** SGDLearner::GetPos (sgd_learner.cc:151-165) */
void GetPos(const SArray<int>& len, SArray<int>* w_pos, SArray<int>* V_pos);

/** sgd::Progress (sgd_utils.h:52-93) */
struct Progress {
  double nrows = 0, loss = 0, auc = 0, penalty = 0, nnz_w = 0;
};

/** the per-batch executor of SGDLearner::IterateData (sgd_learner.cc:201-317) */
class GpuSGDLearner {
 public:
  enum JobType { kTraining = 3, kValidation = 4, kPrediction = 5 };
  /** kwargs: the .conf keys (loss, V_dim, lr, l1, ...), plus `fused` (1: dfx_train_step,
   * batches uploaded through a dfx_feeder; 0: through the Loss/Store interfaces) and `device`.
   * store: a Store holding the model elsewhere (a GpuDistStore worker, dist_store.h; the
   * interface path only); none: a StoreGPU over this learner's GpuSGDUpdater */
  explicit GpuSGDLearner(const KWArgs& kwargs, std::shared_ptr<Store> store = nullptr);
  ~GpuSGDLearner();
  /** one minibatch of raw feature ids; push_cnt = epoch 0 of training with V_dim > 0.
   * Asynchronous on the fused path: the batch is copied into pinned staging and uploaded on
   * the feeder's loader stream; the step runs behind the previous one.  pred (optional):
   * receives the batch's predictions (joins the device), as SavePred writes them.
   * dev_batch (optional, fused path): receives the device batch the feeder uploaded; its
   * buffers are the feeder's, reused by the upload after next, and anything queued on the
   * context's input stream before the next ProcessBatch (a DeviceBatchCache's copies) reads
   * them complete.
   * dev_pred (optional, fused path): receives the device array the step writes the batch's
   * predictions to, in the context stream's order and with no copy down (a DevicePredWriter
   * formats them there); valid until the next Process call. */
  void ProcessBatch(const dmlc::RowBlock<feaid_t>& batch, int job_type, bool push_cnt,
                    std::vector<real_t>* pred = nullptr, dfx_batch* dev_batch = nullptr,
                    const float** dev_pred = nullptr);
  /** the fused path for a batch already on the device (DeviceBatchReader, device_reader.h):
   * dfx_train_step without the pinned copy; the batch's producer is the context's input
   * stream.  pred (optional) receives the predictions (joins the device).  loc (optional): the
   * batch's Localizer outputs from a DeviceBatchCache (dfx_train_step_loc: no Localizer runs).
   * dev_pred (optional): as ProcessBatch's. */
  void ProcessDeviceBatch(const dfx_batch& batch, int job_type, bool push_cnt,
                          std::vector<real_t>* pred = nullptr, const dfx_loc* loc = nullptr,
                          const float** dev_pred = nullptr);
  /** ProcessBatch's upload alone (fused path): the batch on the device, in the feeder's buffers,
   * and no step — the recording pass of epoch_resample=1 copies it into a DeviceBatchCache.
   * UploadDone, after that copy was queued, waits for the context's input stream and frees the
   * feeder's slot (no step's `consumed` mark would). */
  dfx_batch UploadBatch(const dmlc::RowBlock<feaid_t>& batch);
  void UploadDone();
  /** the learner's device context (the fused path's; null when a Store was given) */
  dfx_ctx* context() const { return updater_ ? updater_->context()->h() : nullptr; }
  /** sgd::Progress accumulated since the last call (joins the device) */
  Progress TakeProgress();
  /** the learner's own updater (null when a Store was given) */
  std::shared_ptr<GpuSGDUpdater> updater() const { return updater_; }
  bool fused() const { return fused_; }

 private:
  dfx_batch Upload(const dmlc::RowBlock<feaid_t>& batch);
  bool fused_ = false;
  int V_dim_ = 0;
  std::shared_ptr<GpuSGDUpdater> updater_;
  std::shared_ptr<Store> store_;
  std::unique_ptr<GpuFMLoss> loss_;
  std::unique_ptr<GpuLocalizer> localizer_;
  dfx_feeder* feeder_ = nullptr;
  int64_t feed_rows_ = 0, feed_nnz_ = 0;
  std::unique_ptr<DevArray<float>> dpred_;
  Progress prog_;
};

/** the device batch cache (dfx_batchcache_*, include/difacto_amd.h) of one context: lists of
 * formed batches recorded in the first epoch a run executes and replayed in the later ones */
class DeviceBatchCache {
 public:
  DeviceBatchCache(dfx_ctx* ctx, int64_t budget_bytes, int64_t block_bytes = 0);
  ~DeviceBatchCache();
  DeviceBatchCache(const DeviceBatchCache&) = delete;
  DeviceBatchCache& operator=(const DeviceBatchCache&) = delete;
  void Begin(int64_t list);
  /** a copy of b into the open list; false: the list did not fit and was dropped */
  bool Append(const dfx_batch& b);
  /** closes the open list -> its batch count, -1 if it was dropped */
  int64_t Seal();
  /** a sealed list's batch count; -1 dropped, -2 never begun */
  int64_t Count(int64_t list) const;
  dfx_batch Get(int64_t list, int64_t i) const;
  struct Stats {
    int64_t sealed = 0, dropped = 0, batches = 0, bytes = 0;
  };
  Stats GetStats() const;
  /** after the step that consumed the batch last appended: keeps its Localizer outputs with
   * it; false: they did not fit (the batch stays, the list is not dropped) */
  bool AppendLoc();
  /** the outputs kept with batch i of a sealed list (uniq == NULL: none) */
  dfx_loc GetLoc(int64_t list, int64_t i) const;
  struct LocStats {
    int64_t batches = 0, bytes = 0, served = 0;
  };
  LocStats GetLocStats() const;

  dfx_batchcache* h() const { return h_; }

 private:
  dfx_batchcache* h_ = nullptr;
};

/** a fresh shuffle per epoch of one sealed list of a DeviceBatchCache (dfx_reshuffle_*,
 * include/difacto_amd.h); destroyed before its cache */
class DeviceReshuffler {
 public:
  /** kept() false: the ring and the scratch did not fit the cache's budget */
  DeviceReshuffler(DeviceBatchCache* cache, int64_t list, int64_t batch_rows, int nring = 2);
  ~DeviceReshuffler();
  DeviceReshuffler(const DeviceReshuffler&) = delete;
  DeviceReshuffler& operator=(const DeviceReshuffler&) = delete;
  bool kept() const { return h_ != nullptr; }
  /** the epoch keyed by `key` -> its batch count; -1: the ring no longer fits (replay the list) */
  int64_t BeginEpoch(uint64_t key);
  /** ... without the negative rows this key's draw drops (dfx_reshuffle_begin_epoch_sampled: a
   * fresh down-sample per epoch over a list that holds every row); *rows: the rows kept; -1: the
   * compacted arrays or the ring do not fit (read the part through its reader) */
  int64_t BeginEpochSampled(uint64_t key, float neg_sampling, int64_t* rows);
  /** the next batch, ready by the context's input stream's order; false past the last */
  bool Next(dfx_batch* b);
  /** after the step that took the batch */
  void Consumed();
  struct Stats {
    int64_t rows = 0, batches = 0, ring_bytes = 0, scratch_bytes = 0;
  };
  Stats GetStats() const;

 private:
  dfx_reshuffle* h_ = nullptr;
};

/** SGDLearner::SavePred's rows (sgd_learner.h:72-83), "label\tvalue\n" with value the
 * probability 1 / (1 + exp(-pred)) under pred_prob: the host writer of a prediction file */
void WritePredRows(FILE* f, const real_t* label, const real_t* pred, size_t n, bool pred_prob);

/** the device writer of a prediction file (pred_write=device): the same bytes as WritePredRows,
 * formatted on the device (dfx_predtext_*, include/difacto_amd.h) and written to f as whole
 * batches, batch t while the step of batch t + 1 runs.  A batch with a row the device does not
 * format (csrc/fmtg.h: a field outside 1e-12 <= |x| < 1e12 that is not 0) is written whole by
 * WritePredRows from the slot's copies of its labels and predictions, in its place. */
class DevicePredWriter {
 public:
  DevicePredWriter(dfx_ctx* ctx, FILE* f, bool pred_prob);
  ~DevicePredWriter();
  DevicePredWriter(const DevicePredWriter&) = delete;
  DevicePredWriter& operator=(const DevicePredWriter&) = delete;
  /** batch t: n rows of device labels and predictions, read in the context stream's order,
   * behind the step that wrote pred_dev; both arrays are free again when the call returns or,
   * at the latest, when Submit(t + 1) or Finish returns.  Writes batch t - 1 to the file. */
  void Submit(const float* label_dev, const float* pred_dev, int64_t n);
  /** writes what is still in flight */
  void Finish();
  struct Stats {
    int64_t rows = 0, batches = 0, host_batches = 0;  // host_batches: written by WritePredRows
    double wait_s = 0;                                // the host waited for text
    Stats& operator+=(const Stats& s) {  // over a process's shards
      rows += s.rows;
      batches += s.batches;
      host_batches += s.host_batches;
      wait_s += s.wait_s;
      return *this;
    }
  };
  Stats GetStats() const { return stats_; }

 private:
  void Drain(int slot);
  dfx_predtext* h_ = nullptr;
  FILE* f_;
  bool pred_prob_;
  int next_ = 0;
  bool pending_[2] = {false, false};
  Stats stats_;
};

/** a libsvm reader ("label idx:val ..."): the thin CSR producer the path's caller uses */
bool ReadLibSVM(const std::string& path, RowBlockContainer<feaid_t>* out);

/** rows [begin, end) of a block as a RowBlock view over the same arrays (offsets rebased) */
struct RowSlice {
  std::vector<size_t> offs;
  dmlc::RowBlock<feaid_t> blk;
};
RowSlice Slice(const RowBlockContainer<feaid_t>& c, size_t begin, size_t end);

}  // namespace difacto
#endif  // DIFACTO_AMD_HOST_GPU_ADAPTERS_H_
