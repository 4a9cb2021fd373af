// shard_eval_tests.cc — the sharded stores' evaluation paths, driven from C++:
// GpuShardedStore::Submit(.., DFX_JOB_VALIDATION, .., preds) (dist_host.h, the non-training
// branch of its Run) and GpuSplitLearner::ProcessBatches with its prediction output
// (split_learner.h), against the single context's dfx_train_step(.., DFX_JOB_VALIDATION, ..,
// pred_out) on the same model and rows.  Needs a GPU; run by tests/test_gpu_sharded_eval.py,
// which applies the bounds (this binary prints, and checks only what is exact in C++).
//
// Usage: shard_eval_tests <tests/golden/rcv1_100.libsvm> <scratch dir>
//
// Part 1, per N in {1, 2, 3} x shape x store x pipelined: one model (saved by a short
// single-context training run) loaded into N loopback shards with dfx_store_load_part, one
// validation step on the shape's rows.  Printed per case:
//   case <id> store=<a2a|split> agg=<sum|ranks> pipe=<0|1> N=<n> shape=<name>
//   shard <l> rows <B> nrows <..> loss <%.17g> auc <%.17g>     the shard's progress
//   label <l> ...   pred <l> ...   want <l> ...                 floats as %.9g (round trip)
// Part 2, N = 3: the steps train, train, [flush,] validate, train against the same run without
// the validation step: every shard's dfx_store_pull of every key, compared here bit for bit
// ("seq ... pulls equal"); and the validation step after Flush() against the single context
// loaded from the parts the shards saved at that point (case lines as in part 1).
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "../../difacto_amd/host/dist_host.h"
#include "../../difacto_amd/host/gpu_adapters.h"
#include "../../difacto_amd/host/split_learner.h"

using namespace difacto;

static int g_fail = 0;
#define EXPECT(cond, ...)                                                     \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("  FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);           \
      std::printf(__VA_ARGS__);                                               \
      std::printf("\n");                                                      \
      ++g_fail;                                                               \
    }                                                                         \
  } while (0)

static const char* kKw = "V_dim=4,V_threshold=1,lr=0.1,V_lr=0.05,l1=0.1,seed=7,max_keys=65536";
static const KWArgs kKwArgs = {{"V_dim", "4"}, {"V_threshold", "1"}, {"lr", "0.1"},
                               {"V_lr", "0.05"}, {"l1", "0.1"}, {"seed", "7"},
                               {"max_keys", "65536"}};

static feaid_t ReverseBytes(feaid_t x) {  // include/difacto/base.h:39-51 (test-side)
  x = x << 32 | x >> 32;
  x = (x & 0x0000FFFF0000FFFFULL) << 16 | (x & 0xFFFF0000FFFF0000ULL) >> 16;
  x = (x & 0x00FF00FF00FF00FFULL) << 8 | (x & 0xFF00FF00FF00FF00ULL) >> 8;
  x = (x & 0x0F0F0F0F0F0F0F0FULL) << 4 | (x & 0xF0F0F0F0F0F0F0F0ULL) >> 4;
  return x;
}

// a host row block in device memory
struct DevBlock {
  std::unique_ptr<DevArray<uint64_t>> off, idx;
  std::unique_ptr<DevArray<float>> val, lab;
  dfx_batch b{};
  DevBlock(dfx_ctx* c, const dmlc::RowBlock<feaid_t>& x)
      : off(new DevArray<uint64_t>(c)), idx(new DevArray<uint64_t>(c)),
        val(new DevArray<float>(c)), lab(new DevArray<float>(c)) {
    static const uint64_t zero = 0;
    const size_t B = x.size, nnz = B ? x.offset[B] - x.offset[0] : 0;
    DFX_HOST_CHECK(B == 0 || x.offset[0] == 0, "offsets rebased");
    b.size = (int64_t)B;
    b.nnz = (int64_t)nnz;
    b.offset = B ? off->upload(reinterpret_cast<const uint64_t*>(x.offset), B + 1)
                 : off->upload(&zero, 1);
    b.index = nnz ? idx->upload(x.index, nnz) : nullptr;
    b.value = nnz && x.value ? val->upload(x.value, nnz) : nullptr;
    b.label = B ? lab->upload(x.label, B) : nullptr;
    b.weight = nullptr;
  }
};

struct Rows {
  size_t lo, hi;
};
struct Shape {
  std::string name;
  std::vector<Rows> rows;  // one range per shard
};

static void PrintFloats(const char* what, int l, const float* v, size_t n) {
  std::printf("%s %d", what, l);
  for (size_t i = 0; i < n; ++i) std::printf(" %.9g", v[i]);
  std::printf("\n");
}

// the yardstick: the single context's fused validation step on rows [lo, hi)
static std::vector<float> Yardstick(dfx_ctx* one, const RowBlockContainer<feaid_t>& data,
                                    Rows r) {
  std::vector<float> out(r.hi - r.lo);
  if (out.empty()) return out;
  RowSlice s = Slice(data, r.lo, r.hi);
  DevBlock db(one, s.blk);
  DevArray<float> pred(one);
  pred.ensure(out.size());
  DfxCheck(dfx_train_step(one, &db.b, DFX_JOB_VALIDATION, 0, ~0ull, pred.get()), "dfx_train_step");
  pred.download(out.data(), out.size());
  dfx_progress p;
  DfxCheck(dfx_progress_read(one, &p, 1), "dfx_progress_read");
  return out;
}

static void LoadParts(dfx_ctx* c, const std::string& prefix, int nparts, int rank, int nranks) {
  for (int r = 0; r < nparts; ++r)
    DfxCheck(dfx_store_load_part(c, (prefix + "_part-" + std::to_string(r)).c_str(), rank, nranks),
             "dfx_store_load_part");
}

static void PrintShard(dfx_ctx* c, int l, const RowBlockContainer<feaid_t>& data, Rows r,
                       const std::vector<float>& pred, const std::vector<float>& want) {
  dfx_progress p;
  DfxCheck(dfx_progress_read(c, &p, 1), "dfx_progress_read");
  std::printf("shard %d rows %zu nrows %.0f loss %.17g auc %.17g\n", l, r.hi - r.lo, p.nrows,
              p.loss, p.auc);
  EXPECT(pred.size() == r.hi - r.lo, "shard %d: %zu predictions for %zu rows", l, pred.size(),
         r.hi - r.lo);
  PrintFloats("label", l, data.label.data() + r.lo, r.hi - r.lo);
  PrintFloats("pred", l, pred.data(), pred.size());
  PrintFloats("want", l, want.data(), want.size());
}

// the a2a store over N loopback shards
struct A2a {
  std::vector<dfx_ctx*> ctxs;
  std::unique_ptr<ShardExchange> ex;
  std::unique_ptr<GpuShardedStore> store;
  std::vector<std::unique_ptr<DevBlock>> alive;  // batches live until the store is gone
  A2a(int N, const char* agg, bool pipe) {
    ctxs.assign(N, nullptr);
    const std::string kw = std::string(kKw) + ",push_agg=" + agg;
    for (auto& c : ctxs) DfxCheck(dfx_ctx_create(0, kw.c_str(), &c), "dfx_ctx_create");
    ex = MakeLoopbackExchange(ctxs);
    store.reset(new GpuShardedStore(ex.get(), pipe));
  }
  ~A2a() {
    store.reset();
    alive.clear();
    ex.reset();
    for (auto c : ctxs) dfx_ctx_destroy(c);
  }
  void Submit(const RowBlockContainer<feaid_t>& data, const std::vector<Rows>& rows, int job,
              bool cnt, const std::vector<float*>& preds = {}) {
    std::vector<dfx_batch> bs;
    for (size_t l = 0; l < ctxs.size(); ++l) {
      RowSlice s = Slice(data, rows[l].lo, rows[l].hi);
      alive.emplace_back(new DevBlock(ctxs[l], s.blk));
      bs.push_back(alive.back()->b);
    }
    store->Submit(bs, job, cnt, preds);
  }
};

static std::shared_ptr<GpuSplitLearner> MakeSplit(int N, bool pipe) {
  KWArgs kw = kKwArgs;
  kw.push_back({"pipelined", pipe ? "1" : "0"});
  return GpuSplitLearner::CreateLoopback(N, kw);
}

static void SplitStep(GpuSplitLearner* sl, const RowBlockContainer<feaid_t>& data,
                      const std::vector<Rows>& rows, int job, bool cnt,
                      std::vector<std::vector<real_t>>* preds = nullptr) {
  std::vector<RowSlice> s;
  for (const Rows& r : rows) s.push_back(Slice(data, r.lo, r.hi));
  std::vector<const dmlc::RowBlock<feaid_t>*> ptrs;
  for (auto& x : s) ptrs.push_back(&x.blk);
  sl->ProcessBatches(ptrs, job, cnt, preds);
}

// every key of the data, pulled from one shard: the words a later step would read
static std::vector<float> PullAll(dfx_ctx* c, const std::vector<uint64_t>& keys) {
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
  std::vector<int32_t> lens(keys.size());
  dl.download(lens.data(), lens.size());
  for (int32_t x : lens) v.push_back((float)x);
  return v;
}

static bool SameBits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * 4));
}

int main(int argc, char** argv) {
  RowBlockContainer<feaid_t> data;
  if (argc < 3 || !ReadLibSVM(argv[1], &data)) {
    std::fprintf(stderr, "usage: %s rcv1_100.libsvm <scratch dir>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[2];
  const size_t n = data.Size();
  std::printf("rows %zu\n", n);

  // the model: two epochs of four 25-row batches on one context (counts pushed in epoch 0)
  const std::string model = dir + "/m";
  {
    dfx_ctx* c = nullptr;
    DfxCheck(dfx_ctx_create(0, kKw, &c), "dfx_ctx_create");
    for (int ep = 0; ep < 2; ++ep)
      for (size_t b = 0; b < n; b += 25) {
        RowSlice s = Slice(data, b, std::min(n, b + 25));
        DevBlock db(c, s.blk);
        DfxCheck(dfx_train_step(c, &db.b, DFX_JOB_TRAINING, ep == 0, ~0ull, nullptr),
                 "dfx_train_step");
        DfxCheck(dfx_sync(c), "dfx_sync");
      }
    DfxCheck(dfx_store_save(c, (model + "_part-0").c_str(), 1), "dfx_store_save");
    dfx_ctx_destroy(c);
  }
  dfx_ctx* one = nullptr;
  DfxCheck(dfx_ctx_create(0, kKw, &one), "dfx_ctx_create");
  DfxCheck(dfx_store_load(one, (model + "_part-0").c_str()), "dfx_store_load");

  // ---- part 1: one validation step on a loaded model ---------------------------------------
  std::map<int, std::vector<Shape>> shapes;
  shapes[1] = {{"all", {{0, n}}}};
  shapes[2] = {{"uneven", {{0, 37}, {37, n}}}, {"empty", {{0, n}, {n, n}}}};
  shapes[3] = {{"uneven", {{0, 17}, {17, 61}, {61, n}}}, {"empty", {{0, 41}, {41, 41}, {41, n}}}};
  int id = 0;
  for (int N = 1; N <= 3; ++N) {
    for (const Shape& sh : shapes[N]) {
      std::vector<std::vector<float>> want;
      for (const Rows& r : sh.rows) want.push_back(Yardstick(one, data, r));
      for (int pipe = 0; pipe < 2; ++pipe) {
        for (const char* agg : {"sum", "ranks"}) {
          std::printf("case %d store=a2a agg=%s pipe=%d N=%d shape=%s\n", id++, agg, pipe, N,
                      sh.name.c_str());
          A2a s(N, agg, pipe != 0);
          std::vector<std::unique_ptr<DevArray<float>>> dp;
          std::vector<float*> pp;
          for (int l = 0; l < N; ++l) {
            LoadParts(s.ctxs[l], model, 1, l, N);
            dp.emplace_back(new DevArray<float>(s.ctxs[l]));
            dp.back()->ensure(sh.rows[l].hi - sh.rows[l].lo);
            pp.push_back(dp.back()->get());
          }
          s.Submit(data, sh.rows, DFX_JOB_VALIDATION, false, pp);
          s.store->Flush();  // pipelined: the submitted step runs here
          for (int l = 0; l < N; ++l) {
            std::vector<float> pred(sh.rows[l].hi - sh.rows[l].lo);
            dp[l]->download(pred.data(), pred.size());
            PrintShard(s.ctxs[l], l, data, sh.rows[l], pred, want[l]);
          }
          dp.clear();
        }
        std::printf("case %d store=split agg=sum pipe=%d N=%d shape=%s\n", id++, pipe, N,
                    sh.name.c_str());
        std::shared_ptr<GpuSplitLearner> sl = MakeSplit(N, pipe != 0);
        for (int l = 0; l < N; ++l) LoadParts(sl->shard(l), model, 1, l, N);
        std::vector<std::vector<real_t>> preds;
        SplitStep(sl.get(), data, sh.rows, GpuSplitLearner::kValidation, false, &preds);
        EXPECT((int)preds.size() == N, "split: %zu prediction vectors", preds.size());
        for (int l = 0; l < N; ++l)
          PrintShard(sl->shard(l), l, data, sh.rows[l], preds[l], want[l]);
      }
    }
  }

  // ---- part 2: train, train, [flush,] validate, train -------------------------------------
  std::set<uint64_t> kset;
  for (feaid_t x : data.index) kset.insert(ReverseBytes(x));
  const std::vector<uint64_t> keys(kset.begin(), kset.end());
  const int N = 3;
  // four steps' rows per shard: unequal counts, and shard 1 idle in the validation step
  const std::vector<std::vector<Rows>> st = {{{0, 10}, {10, 17}, {17, 30}},
                                             {{30, 34}, {34, 50}, {50, 55}},
                                             {{55, 70}, {70, 70}, {70, 81}},
                                             {{81, 90}, {90, 91}, {91, n}}};
  for (int pipe = 0; pipe < 2; ++pipe) {
    for (const char* cfg : {"a2a sum", "a2a ranks", "split sum"}) {
      const bool split = cfg[0] == 's';
      const char* agg = std::strchr(cfg, ' ') + 1;
      // mode 0: no validation step; 1: flush, validate (with predictions), then go on;
      // 2: the validation step queued between the training steps, no flush around it
      std::vector<std::vector<float>> pulls[3];
      for (int mode = 0; mode < 3; ++mode) {
        std::unique_ptr<A2a> a;
        std::shared_ptr<GpuSplitLearner> sl;
        if (split)
          sl = MakeSplit(N, pipe != 0);
        else
          a.reset(new A2a(N, agg, pipe != 0));
        auto ctx = [&](int l) { return split ? sl->shard(l) : a->ctxs[l]; };
        auto train = [&](int t) {
          if (split)
            SplitStep(sl.get(), data, st[t], GpuSplitLearner::kTraining, t == 0);
          else
            a->Submit(data, st[t], DFX_JOB_TRAINING, t == 0);
        };
        auto flush = [&]() {
          if (split)
            sl->Flush();
          else
            a->store->Flush();
        };
        train(0);
        train(1);
        if (mode != 2) flush();
        if (mode == 1) {
          // the validation step after Flush() sees the last push: the yardstick is a single
          // context loaded from the parts the shards hold now
          std::printf("case %d store=%s agg=%s pipe=%d N=%d shape=after_flush\n", id++,
                      split ? "split" : "a2a", agg, pipe, N);
          std::vector<std::vector<real_t>> preds(N);
          for (int l = 0; l < N; ++l) {  // the training steps' progress is not the case's
            dfx_progress p;
            DfxCheck(dfx_progress_read(ctx(l), &p, 1), "dfx_progress_read");
          }
          if (split) {
            SplitStep(sl.get(), data, st[2], GpuSplitLearner::kValidation, false, &preds);
          } else {
            std::vector<std::unique_ptr<DevArray<float>>> dp;
            std::vector<float*> pp;
            for (int l = 0; l < N; ++l) {
              dp.emplace_back(new DevArray<float>(ctx(l)));
              dp.back()->ensure(st[2][l].hi - st[2][l].lo);
              pp.push_back(dp.back()->get());
            }
            a->Submit(data, st[2], DFX_JOB_VALIDATION, false, pp);
            a->store->Flush();
            for (int l = 0; l < N; ++l) {
              preds[l].resize(st[2][l].hi - st[2][l].lo);
              dp[l]->download(preds[l].data(), preds[l].size());
            }
          }
          const std::string now = dir + "/seq";
          dfx_ctx* y = nullptr;
          DfxCheck(dfx_ctx_create(0, kKw, &y), "dfx_ctx_create");
          for (int l = 0; l < N; ++l) {
            DfxCheck(dfx_sync(ctx(l)), "dfx_sync");
            DfxCheck(dfx_store_save(ctx(l), (now + "_part-" + std::to_string(l)).c_str(), 0),
                     "dfx_store_save");
          }
          LoadParts(y, now, N, 0, 1);
          for (int l = 0; l < N; ++l)
            PrintShard(ctx(l), l, data, st[2][l], preds[l], Yardstick(y, data, st[2][l]));
          dfx_ctx_destroy(y);
        } else if (mode == 2) {
          if (split)
            SplitStep(sl.get(), data, st[2], GpuSplitLearner::kValidation, false);
          else
            a->Submit(data, st[2], DFX_JOB_VALIDATION, false);
        }
        train(3);
        flush();
        for (int l = 0; l < N; ++l) {
          DfxCheck(dfx_sync(ctx(l)), "dfx_sync");
          pulls[mode].push_back(PullAll(ctx(l), keys));
        }
      }
      for (int mode = 1; mode < 3; ++mode) {
        bool same = true;
        for (int l = 0; l < N; ++l) same = same && SameBits(pulls[mode][l], pulls[0][l]);
        EXPECT(same, "%s pipe=%d mode %d: a validation step changed the model", cfg, pipe, mode);
        std::printf("seq %s pipe=%d mode=%d pulls %s (%zu keys)\n", cfg, pipe, mode,
                    same ? "equal" : "DIFFER", keys.size());
      }
    }
  }
  dfx_ctx_destroy(one);
  std::printf(g_fail ? "FAILED (%d)\n" : "ALL PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
