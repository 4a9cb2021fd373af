// split_device_tests.cc — GpuSplitLearner::ProcessDeviceBatches (split_learner.h) from C++ on
// loopback N = 3 and N = 1: steps fed device batches, mixed steps and recorded-then-replayed
// steps against the same steps fed host row blocks.  Needs a GPU; run by
// tests/test_gpu_split_device.py.  Every comparison is exact (bits), so it is made here.
//
// Usage: split_device_tests
//
// Batches: 7, 64 and 65 rows of 1-40 distinct ids out of a pool of 400 plus one hot id that
// every row holds, labels +-1; valued (x in (0, 1]) and binary.  Learners: FM with V_dim = 4
// and logit, pipelined 0 and 1 (N = 1: 1).  A run is a schedule of steps (per local worker a
// batch or none), counts pushed in the first two, then one validation step with predictions,
// then one more training step; its result is every shard's dfx_store_pull of every id, the
// training and the validation progress of every shard, and the validation predictions.
//   (a) host      every item a host block — the yardstick of its schedule, run twice: (0)
//       device    the same batches as device arrays after the first step
//   (b) mixed     N = 3: worker 0 device, worker 1 host, worker 2 none in every step
//   (c) the validation predictions of the device runs against the host run's, bit for bit
//   (d) record    host items with dev_out appended to a DeviceBatchCache per shard; the cached
//                 batches copied back equal the host blocks byte for byte
//       replay    ... and the schedule run a second time from the caches equals the host run of
//                 the doubled schedule
//   (e) alternate 12 pipelined steps, host and device items alternating per worker and step,
//                 on the learner's 3 staging slots
// Printed per comparison: "<case> <what> equal|DIFFER".
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>

#include "../../difacto_amd/host/gpu_adapters.h"
#include "../../difacto_amd/host/split_learner.h"

using namespace difacto;

static int g_fail = 0;
static void Report(const std::string& name, const char* what, bool same) {
  std::printf("%s %s %s\n", name.c_str(), what, same ? "equal" : "DIFFER");
  if (!same) ++g_fail;
}

static feaid_t ReverseBytes(feaid_t x) {  // include/difacto/base.h:39-51 (test-side)
  x = x << 32 | x >> 32;
  x = (x & 0x0000FFFF0000FFFFULL) << 16 | (x & 0xFFFF0000FFFF0000ULL) >> 16;
  x = (x & 0x00FF00FF00FF00FFULL) << 8 | (x & 0xFF00FF00FF00FF00ULL) >> 8;
  x = (x & 0x0F0F0F0F0F0F0F0FULL) << 4 | (x & 0xF0F0F0F0F0F0F0F0ULL) >> 4;
  return x;
}

struct Data {
  std::vector<feaid_t> pool;  // pool[0] is the hot id
  std::vector<RowBlockContainer<feaid_t>> batch;
};

static Data MakeData(bool valued, int nbatches) {
  Data d;
  std::mt19937_64 rng(valued ? 11 : 12);
  std::set<feaid_t> seen;
  while (d.pool.size() < 401) {
    const feaid_t k = rng();
    if (k != ~0ull && ReverseBytes(k) != ~0ull && seen.insert(k).second) d.pool.push_back(k);
  }
  const size_t sizes[3] = {7, 64, 65};
  d.batch.resize(nbatches);
  for (int b = 0; b < nbatches; ++b) {
    RowBlockContainer<feaid_t>& c = d.batch[b];
    for (size_t r = 0; r < sizes[b % 3]; ++r) {
      const size_t len = 1 + rng() % 40;
      std::set<size_t> ids{0};
      while (ids.size() < len) ids.insert(1 + rng() % 400);
      for (size_t i : ids) {
        c.index.push_back(d.pool[i]);
        if (valued) c.value.push_back((float)(1 + rng() % 1000) / 1000.f);
      }
      c.offset.push_back(c.index.size());
      c.label.push_back(rng() % 3 == 0 ? 1.f : -1.f);
    }
  }
  return d;
}

// a host row block in device memory, uploaded on the context's stream (join it before use)
struct DevBlock {
  std::unique_ptr<DevArray<uint64_t>> off, idx;
  std::unique_ptr<DevArray<float>> val, lab;
  dfx_batch b{};
  DevBlock(dfx_ctx* c, const RowBlockContainer<feaid_t>& x)
      : off(new DevArray<uint64_t>(c)), idx(new DevArray<uint64_t>(c)),
        val(new DevArray<float>(c)), lab(new DevArray<float>(c)) {
    const size_t B = x.Size(), nnz = x.index.size();
    b.size = (int64_t)B;
    b.nnz = (int64_t)nnz;
    b.offset = off->upload(reinterpret_cast<const uint64_t*>(x.offset.data()), B + 1);
    b.index = idx->upload(x.index.data(), nnz);
    b.value = x.value.empty() ? nullptr : val->upload(x.value.data(), nnz);
    b.label = lab->upload(x.label.data(), B);
    b.weight = nullptr;
  }
};

enum Kind { kHost, kDev, kNone };
// sched[t][l]: the batch of worker l in step t, -1: none
typedef std::vector<std::vector<int>> Sched;

struct Result {
  std::vector<std::vector<float>> pulls;      // per shard
  std::vector<std::vector<double>> progress;  // per shard: train {n, loss, auc}, val {..}
  std::vector<std::vector<real_t>> preds;     // the validation step's
  bool copies_equal = true;                   // record mode: the cached batches
};

// (the lengths are written only with V_dim > 0: a logit record is its one word)
static std::vector<float> PullAll(dfx_ctx* c, const std::vector<uint64_t>& keys, bool fm) {
  DevArray<uint64_t> dk(c);
  DevArray<float> dv(c);
  DevArray<int32_t> dl(c);
  dk.upload(keys.data(), keys.size());
  dv.ensure(keys.size() * 5);
  dl.ensure(keys.size());
  int64_t nv = 0;
  DfxCheck(dfx_store_pull(c, dk.get(), (int64_t)keys.size(), dv.get(), dl.get(), &nv),
           "dfx_store_pull");
  std::vector<float> v((size_t)nv);
  dv.download(v.data(), v.size());
  if (!fm) return v;
  std::vector<int32_t> lens(keys.size());
  dl.download(lens.data(), lens.size());
  for (int32_t x : lens) v.push_back((float)x);
  return v;
}

template <typename T>
static bool SameBytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() &&
         (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// *what: "all", or the parts that differ
static bool Same(const Result& a, const Result& b, const char** what) {
  bool pulls = a.pulls.size() == b.pulls.size(), prog = a.progress.size() == b.progress.size(),
       preds = a.preds.size() == b.preds.size();
  for (size_t l = 0; pulls && l < a.pulls.size(); ++l) pulls = SameBytes(a.pulls[l], b.pulls[l]);
  for (size_t l = 0; prog && l < a.progress.size(); ++l)
    prog = SameBytes(a.progress[l], b.progress[l]);
  for (size_t l = 0; preds && l < a.preds.size(); ++l) preds = SameBytes(a.preds[l], b.preds[l]);
  static const char* names[8] = {"pulls+progress+predictions", "progress+predictions",
                                 "pulls+predictions", "predictions", "pulls+progress",
                                 "progress", "pulls", "all"};
  *what = names[(pulls ? 1 : 0) | (prog ? 2 : 0) | (preds ? 4 : 0)];
  return pulls && prog && preds;
}

// device -> host of n elements, after the whole device is idle
template <typename T>
static std::vector<T> Back(dfx_ctx* c, const T* p, size_t n) {
  std::vector<T> v(n);
  if (n) DfxCheck(dfx_memcpy(c, v.data(), p, n * sizeof(T), 1), "dfx_memcpy");
  return v;
}

static bool EqualsHost(dfx_ctx* c, const dfx_batch& b, const RowBlockContainer<feaid_t>& x) {
  if (b.size != (int64_t)x.Size() || b.nnz != (int64_t)x.index.size()) return false;
  if ((b.value != nullptr) != !x.value.empty() || b.weight != nullptr) return false;
  std::vector<uint64_t> off(x.offset.begin(), x.offset.end());
  bool ok = SameBytes(Back(c, b.offset, off.size()), off);
  ok = ok && SameBytes(Back(c, b.index, x.index.size()), x.index);
  ok = ok && SameBytes(Back(c, b.label, x.label.size()), x.label);
  if (b.value) ok = ok && SameBytes(Back(c, b.value, x.value.size()), x.value);
  return ok;
}

static Kind AllHost(int, int) { return kHost; }
static Kind DevAfterFirst(int t, int) { return t == 0 ? kHost : kDev; }
static Kind Mixed(int, int l) { return l == 0 ? kDev : l == 1 ? kHost : kNone; }
static Kind Alternate(int t, int l) { return (t + l) % 2 ? kDev : kHost; }

// kind(t, l) of the training steps; the validation step and the last training step take the
// kind of step 1.  record: dev_out of every step goes into a cache per shard, and `replays`
// further passes over the schedule come from the caches
static Result Run(const Data& d, int N, const char* loss, bool pipe, const Sched& sched,
                  Kind (*kind)(int, int), bool record = false, int replays = 0) {
  KWArgs kw = {{"V_dim", std::strcmp(loss, "fm") ? "0" : "4"}, {"V_threshold", "1"},
               {"lr", "0.1"}, {"V_lr", "0.05"}, {"l1", "0.1"}, {"seed", "7"},
               {"max_keys", "65536"}, {"loss", loss}, {"pipelined", pipe ? "1" : "0"}};
  std::shared_ptr<GpuSplitLearner> sl = GpuSplitLearner::CreateLoopback(N, kw);
  Result out;
  {
    // every batch of every worker in device memory before the first step (the steps wait for
    // the contexts' input streams only)
    std::vector<std::vector<std::unique_ptr<DevBlock>>> dev(N);
    for (int l = 0; l < N; ++l) {
      for (const auto& b : d.batch) dev[l].emplace_back(new DevBlock(sl->shard(l), b));
      DfxCheck(dfx_sync(sl->shard(l)), "dfx_sync");
    }
    std::vector<std::unique_ptr<DeviceBatchCache>> caches;
    if (record)
      for (int l = 0; l < N; ++l) {
        caches.emplace_back(new DeviceBatchCache(sl->shard(l), (int64_t)64 << 20, 1 << 20));
        caches[l]->Begin(0);
      }
    std::vector<dmlc::RowBlock<feaid_t>> blk(N);
    const RowBlockContainer<feaid_t> empty;
    std::vector<std::vector<int>> recorded(N);
    auto step = [&](const std::vector<int>& w, int t, int job, bool cnt,
                    std::vector<std::vector<real_t>>* preds, bool rec) {
      std::vector<GpuSplitLearner::Item> it(N);
      for (int l = 0; l < N; ++l) {
        if (w[l] < 0) {  // an all-host run gives an empty host block, any other none
          if (kind == AllHost) {
            blk[l] = empty.GetBlock();
            it[l].host = &blk[l];
          }
          continue;
        }
        if (kind(t, l) == kHost) {
          blk[l] = d.batch[w[l]].GetBlock();
          it[l].host = &blk[l];
        } else if (kind(t, l) == kDev) {
          it[l].dev = &dev[l][w[l]]->b;
        }
      }
      std::vector<dfx_batch> up;
      sl->ProcessDeviceBatches(it, job, cnt, preds, rec ? &up : nullptr);
      for (int l = 0; rec && l < N; ++l)
        if (it[l].host && w[l] >= 0) {
          caches[l]->Append(up[l]);
          recorded[l].push_back(w[l]);
        }
    };
    const int T = (int)sched.size();
    for (int t = 0; t < T; ++t)
      step(sched[t], t, GpuSplitLearner::kTraining, t < 2, nullptr, record);
    std::vector<int64_t> n_cached(N, 0);
    if (record)
      for (int l = 0; l < N; ++l) n_cached[l] = caches[l]->Seal();
    for (int r = 0; r < replays; ++r) {
      std::vector<int64_t> pos(N, 0);
      for (int t = 0; t < T; ++t) {
        std::vector<GpuSplitLearner::Item> it(N);
        std::vector<dfx_batch> got(N);
        for (int l = 0; l < N; ++l) {
          if (sched[t][l] < 0) continue;
          got[l] = caches[l]->Get(0, pos[l]++);
          it[l].dev = &got[l];
        }
        sl->ProcessDeviceBatches(it, GpuSplitLearner::kTraining, false);
      }
    }
    out.progress.resize(N);
    for (int l = 0; l < N; ++l) {
      const Progress p = sl->TakeProgress(l);
      out.progress[l] = {p.nrows, p.loss, p.auc};
    }
    step(sched[T > 1 ? 1 : 0], 1, GpuSplitLearner::kValidation, false, &out.preds, false);
    for (int l = 0; l < N; ++l) {
      const Progress p = sl->TakeProgress(l);
      out.progress[l].insert(out.progress[l].end(), {p.nrows, p.loss, p.auc});
    }
    step(sched[0], 1, GpuSplitLearner::kTraining, false, nullptr, false);
    sl->Sync();
    if (record) {
      DFX_HOST_CHECK(hipDeviceSynchronize() == hipSuccess, "hipDeviceSynchronize");
      for (int l = 0; l < N; ++l) {
        out.copies_equal = out.copies_equal && n_cached[l] == (int64_t)recorded[l].size();
        for (int64_t i = 0; out.copies_equal && i < n_cached[l]; ++i)
          out.copies_equal = EqualsHost(sl->shard(l), caches[l]->Get(0, i),
                                        d.batch[recorded[l][i]]);
      }
    }
    std::vector<uint64_t> keys;
    for (feaid_t k : d.pool) keys.push_back(ReverseBytes(k));
    for (int l = 0; l < N; ++l) {
      DfxCheck(dfx_sync(sl->shard(l)), "dfx_sync");
      out.pulls.push_back(PullAll(sl->shard(l), keys, !std::strcmp(loss, "fm")));
    }
    // the caches and the device arrays go before the learner's contexts
  }
  sl.reset();
  return out;
}

int main() {
  for (int valued = 0; valued < 2; ++valued) {
    const int nb = 9;
    const Data d = MakeData(valued != 0, nb);
    for (const char* loss : {"fm", "logit"}) {
      for (int N : {3, 1}) {
        // 4 steps; the workers' batch sizes differ within a step
        Sched s4, s12, smix;
        for (int t = 0; t < 12; ++t) {
          std::vector<int> w(N);
          for (int l = 0; l < N; ++l) w[l] = (t * 2 + l) % nb;
          if (t < 4) s4.push_back(w);
          s12.push_back(w);
          if (N == 3) w[2] = -1;
          if (t < 4) smix.push_back(w);
        }
        Sched s8 = s4;
        s8.insert(s8.end(), s4.begin(), s4.end());
        for (int pipe = N == 1 ? 1 : 0; pipe < 2; ++pipe) {  // N = 1: the pipelined schedule only
          const std::string name = std::string("valued=") + (valued ? "1" : "0") + " loss=" +
                                   loss + " N=" + std::to_string(N) + " pipe=" +
                                   std::to_string(pipe);
          const char* what = nullptr;
          const Result host = Run(d, N, loss, pipe != 0, s4, AllHost);
          bool nonzero = false;
          for (const auto& p : host.pulls)
            for (float x : p) nonzero = nonzero || x != 0;
          Report(name, "(host run trained: some pulled word is not 0)", nonzero);
          // the yardstick is the same bits in every run
          const Result again = Run(d, N, loss, pipe != 0, s4, AllHost);
          Report(name + " (0) host twice", Same(host, again, &what) ? "all" : what,
                 Same(host, again, &what));
          const Result dev = Run(d, N, loss, pipe != 0, s4, DevAfterFirst);
          Report(name + " (a) device", Same(host, dev, &what) ? "all" : what,
                 Same(host, dev, &what));
          Report(name + " (c) device", "predictions",
                 host.preds.size() == dev.preds.size() && !host.preds.empty() &&
                     !host.preds[0].empty() && Same(host, dev, &what));
          if (N == 3) {
            const Result mh = Run(d, N, loss, pipe != 0, smix, AllHost);
            const Result mx = Run(d, N, loss, pipe != 0, smix, Mixed);
            const bool same = Same(mh, mx, &what);
            Report(name + " (b) mixed", what, same);
            Report(name + " (b) mixed", "(the idle worker has no rows)",
                   mx.preds.size() == 3 && mx.preds[2].empty() && mx.progress[2][0] == 0);
          }
          const Result h8 = Run(d, N, loss, pipe != 0, s8, AllHost);
          const Result rep = Run(d, N, loss, pipe != 0, s4, AllHost, true, 1);
          Report(name + " (d) record", "cached copies", rep.copies_equal);
          Report(name + " (d) replay", Same(h8, rep, &what) ? "all" : what, Same(h8, rep, &what));
          if (pipe) {
            const Result h12 = Run(d, N, loss, true, s12, AllHost);
            const Result alt = Run(d, N, loss, true, s12, Alternate);
            Report(name + " (e) alternate", Same(h12, alt, &what) ? "all" : what,
                   Same(h12, alt, &what));
          }
        }
      }
    }
  }
  std::printf(g_fail ? "FAILED (%d)\n" : "ALL PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
