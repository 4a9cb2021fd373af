// split_learner.h — SGDLearner::IterateData's per-batch executor (sgd_learner.cc:201-317) on
// N GPUs through the owner-computes split (libdfx_dist.so, include/difacto_amd_dist.h): the
// multi-GPU counterpart of GpuSGDLearner(fused=1).
//
// The reference's worker loop pulls weights from KVStoreDist servers, predicts, computes the
// gradient and pushes it (store.h:55-83, kvstore_dist.h:90-175).  That Store contract moves
// every touched key's record across the links twice per step; the split moves per-row
// partials instead and runs each key's forward / backward / update on the GPU that owns it.
// So the drop-in point for the fast multi-GPU path is the Learner, one level above Store:
// GpuSplitLearner takes the worker's raw minibatch, exactly what IterateData's executor
// receives from its reader thread, and one step of every worker is one synchronous reference
// step on the concatenation of their batches in rank order (push_agg=sum).
//
//   loopback  N workers held by one process (one thread each, on one GPU: the tests)
//   RCCL      one worker per process (torchrun / the reference's launcher: RANK, WORLD_SIZE,
//             LOCAL_RANK; communicator ids through the node-local id file, dist_host.h)
//
// Every worker gives one batch per step (ProcessBatch; an idle worker an empty batch), with
// the same job type and count-push flag (lockstep, as the synchronous mode requires).  The
// batch is copied into pinned staging (the caller may reuse it on return) and uploaded on a
// loader stream; the step runs asynchronously, pipelined behind the previous one.  The
// servers' tables grow at the steps' sync points as the model grows (sgd_updater.h:178).
#ifndef DIFACTO_AMD_HOST_SPLIT_LEARNER_H_
#define DIFACTO_AMD_HOST_SPLIT_LEARNER_H_

#include <functional>
#include <memory>
#include <vector>

#include "gpu_adapters.h"

namespace difacto {

class GpuSplitLearner {
 public:
  enum JobType { kTraining = 3, kValidation = 4, kPrediction = 5 };
  /** kwargs: the .conf keys of every shard (loss, V_dim, lr, l1, V_threshold, ..., max_keys),
   * plus `pipelined` (1: step t+1's partition / key exchange / owner Localizer beside step t)
   * and `slices` (dfx_split_store_set_slices) */
  static std::shared_ptr<GpuSplitLearner> CreateLoopback(int nshards, const KWArgs& kwargs);
  static std::shared_ptr<GpuSplitLearner> CreateRccl(const KWArgs& kwargs);
  ~GpuSplitLearner();

  int nlocal() const;
  int nranks() const;
  int rank(int local) const;
  /** the server context of local shard l (model save / load / stats) */
  dfx_ctx* shard(int local) const;
  /** worker `local`'s minibatch of this step (thread-safe across the local workers: the step
   * is submitted when the last of them gave its batch; the others wait for that).
   * pred (optional; validation and prediction jobs only): the batch's predictions, one per
   * row, as SGDLearner's executor hands them to SavePred (sgd_learner.cc:231-237).  A step any
   * of whose workers asks for them runs before the calls return (submit, then flush: an
   * evaluation step pushes nothing, so no schedule depends on when it runs), and every
   * worker's vector is filled on return. */
  void ProcessBatch(int local, const dmlc::RowBlock<feaid_t>& batch, int job_type,
                    bool push_cnt, std::vector<real_t>* pred = nullptr);
  /** one step from a single caller thread: batches[l] is local worker l's minibatch;
   * preds (optional, as above): resized to one vector per local worker */
  void ProcessBatches(const std::vector<const dmlc::RowBlock<feaid_t>*>& batches, int job_type,
                      bool push_cnt, std::vector<std::vector<real_t>>* preds = nullptr);
  /** a local worker's batch of one step: a host row block (staged and uploaded, as
   * ProcessBatches'), or a batch in device memory (ready by the context's input stream's
   * order; a DeviceBatchCache's, alive until the learner is gone, or one alive until its release
   * hook is called), or neither: an empty batch.
   * The input stream: the learner makes its feeders, whose loader stream replaces the context's
   * input stream, only when a step holds a host item (Impl::Feeders).  A caller that keeps a
   * DeviceTextFeed on a shard's context gives that shard no host item while the feed lives, so
   * the input stream stays the feed's: its gathers, a cache's Append copies and the store's wait
   * for the device items are ordered by it. */
  struct Item {
    const dmlc::RowBlock<feaid_t>* host = nullptr;
    const dfx_batch* dev = nullptr;
    /** a device item whose arrays the owner reuses (a DeviceTextFeed's ring entry or text
     * slot): called on the submitting thread once the item's last reader, the step's combine on
     * the context stream, has been queued — inside this call when pipelined=0, inside the next
     * submit or the flush (Flush, Sync, a step that asks for predictions) when pipelined=1.
     * An event recorded on the context stream from the hook is behind that reader. */
    std::function<void()> release;
  };
  /** one step from a single caller thread, like ProcessBatches (its all-host case); host and
   * device items may be mixed in a step.  A device item goes to the split store as it is: no
   * staging, no copy, and no staging slot is held for it.  preds: as above, the sizes are the
   * batches' own.
   * dev_out (optional): resized to one dfx_batch per local worker; dev_out[l] is the device
   * batch worker l's host block was uploaded into (a device item: itself; none: size 0), valid
   * until the worker's next host item is staged — what GpuSGDLearner::ProcessBatch's dev_out is.
   * A caller that records appends it to the shard's DeviceBatchCache right after the call: the
   * cache copies on the context's input stream, which is the feeder's loader stream (the feeder
   * installs it, dfx_feeder_create_slots), so the copy runs behind the upload and before the
   * next upload into the same slot with no event and no host wait.
   * The contexts are the learner's own, and a cache must go before its context: a caller
   * first joins the learner (Sync: no queued step reads a cached batch any more), then
   * destroys its caches, then the learner.
   * dev_preds (optional, evaluation jobs): resized to one pointer per local worker; the step
   * runs before the call returns as with preds, and dev_preds[l] is the device array holding
   * worker l's predictions (dev_out[l].size of them) in its context stream's order, with no copy
   * down; valid until the next step.  A DevicePredWriter formats them there. */
  void ProcessDeviceBatches(const std::vector<Item>& items, int job_type, bool push_cnt,
                            std::vector<std::vector<real_t>>* preds = nullptr,
                            std::vector<dfx_batch>* dev_out = nullptr,
                            std::vector<const float*>* dev_preds = nullptr);
  /** run the queued step (one thread, every local worker idle) */
  void Flush();
  /** Flush, then wait for every context and stream of the split driver: nothing reads a
   * submitted batch any more */
  void Sync();
  /** host seconds the split store waited on its run-ahead bound (pipelined) since the last call */
  double TakeThrottleSeconds();
  /** sgd::Progress of worker `local` since the last call (Flush first) */
  Progress TakeProgress(int local);
  /** v summed over the processes (the thread that submits steps; a collective of every rank,
   * ordered with the steps' own exchanges, so it needs no flush) */
  void AllReduceSum(std::vector<double>* v);

  struct Impl;

 private:
  explicit GpuSplitLearner(std::unique_ptr<Impl> impl);
  std::unique_ptr<Impl> impl_;
};

}  // namespace difacto
#endif  // DIFACTO_AMD_HOST_SPLIT_LEARNER_H_
