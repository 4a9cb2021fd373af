// shard_parse_tests.cc — both sharded stores fed by DeviceBatchReaders (device_reader.h) from
// C++ on loopback N = 3, against the same stores fed the host reader's blocks.  Needs a GPU; run
// by tests/test_gpu_shard_parse.py.  Every comparison is exact (bits), so it is made here.
//
// Usage: shard_parse_tests <rcv1_100.libsvm> <criteo text, 500 rows> <scratch dir>
//
// A run: two jobs of training (shard l reads part j * N + l of 2 N in batches of 5, shuffle
// buffer 15, neg_sampling 0.8, counts pushed in the first two steps), a flush, the shards'
// progress, then two jobs of validation (every chunk one batch), a flush, the progress, and
// every shard's model saved with its aux words (compared entry by entry, every byte of each).
// chunk_bytes = 4096, so a part is many chunks: the feeds' 4 text slots and 4 ring entries are
// each reused many times, with the stores' marks one step late when pipelined and the readers
// of a job gone before its last batches are marked.  Stores: GpuShardedStore (a2a) and GpuSplitLearner (split), pipelined 0 and 1.
//   host    BatchReader / TextReader blocks (a2a: uploaded; split: host items)
//   device  DeviceBatchReader batches on one DeviceTextFeed per shard, marked as
//           dfx_train's runners mark them: a2a by the caller after the Submit that ran the
//           step, split by the learner's release hook
// Printed per comparison: "<case> <what> equal|DIFFER".  The last case omits the marks and
// expects the reader's FeedProtocolError, in minibatch mode (the ring) and in whole-chunk mode
// (the slots): a host-side throw, nothing is queued wrongly.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>

#include "../../difacto_amd/host/device_reader.h"
#include "../../difacto_amd/host/dist_host.h"
#include "../../difacto_amd/host/gpu_adapters.h"
#include "../../difacto_amd/host/split_learner.h"

using namespace difacto;

static int g_fail = 0;
static void Report(const std::string& name, const char* what, bool same) {
  std::printf("%s %s %s\n", name.c_str(), what, same ? "equal" : "DIFFER");
  if (!same) ++g_fail;
}

static const int N = 3, kJobs = 2, kDepth = 4;
static const size_t kBatch = 5, kShuf = 15, kChunk = 4096;
static const float kNeg = 0.8f;

// a host row block in device memory (the a2a store takes device batches)
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
    static const uint64_t zero = 0;
    b.offset = B ? off->upload(reinterpret_cast<const uint64_t*>(x.offset.data()), B + 1)
                 : off->upload(&zero, 1);
    b.index = nnz ? idx->upload(x.index.data(), nnz) : nullptr;
    b.value = x.value.empty() ? nullptr : val->upload(x.value.data(), nnz);
    b.label = B ? lab->upload(x.label.data(), B) : nullptr;
  }
};

// a shard's batch of a step: a host block, a feed's batch, or neither
struct Src {
  const RowBlockContainer<feaid_t>* host = nullptr;
  const dfx_batch* dev = nullptr;
  DeviceTextFeed* feed = nullptr;
  uint64_t ticket = 0;
};

struct Driver {
  virtual ~Driver() {}
  virtual dfx_ctx* ctx(int l) = 0;
  virtual void Step(const std::vector<Src>& src, int job, bool cnt) = 0;
  virtual void Flush() = 0;
};

struct A2aDriver : Driver {
  struct Mark {
    DeviceTextFeed* feed;
    uint64_t ticket;
  };
  bool pipe;
  std::vector<dfx_ctx*> ctxs;
  std::unique_ptr<ShardExchange> ex;
  std::unique_ptr<GpuShardedStore> store;
  std::vector<std::unique_ptr<DevBlock>> alive;  // host blocks live until the store is gone
  std::vector<Mark> queued;
  A2aDriver(const std::string& kw, bool p) : pipe(p) {
    ctxs.assign(N, nullptr);
    for (auto& c : ctxs) DfxCheck(dfx_ctx_create(0, kw.c_str(), &c), "dfx_ctx_create");
    ex = MakeLoopbackExchange(ctxs);
    store.reset(new GpuShardedStore(ex.get(), pipe));
  }
  ~A2aDriver() override {
    store.reset();
    alive.clear();
    ex.reset();
    for (auto c : ctxs) dfx_ctx_destroy(c);
  }
  dfx_ctx* ctx(int l) override { return ctxs[l]; }
  static void MarkAll(std::vector<Mark>* v) {
    for (const Mark& m : *v) m.feed->Mark(m.ticket);
    v->clear();
  }
  void Step(const std::vector<Src>& src, int job, bool cnt) override {
    static const RowBlockContainer<feaid_t> empty;
    std::vector<dfx_batch> bs(N);
    std::vector<Mark> now;
    for (int l = 0; l < N; ++l) {
      if (src[l].dev) {
        bs[l] = *src[l].dev;
        now.push_back(Mark{src[l].feed, src[l].ticket});
      } else {
        alive.emplace_back(new DevBlock(ctxs[l], src[l].host ? *src[l].host : empty));
        bs[l] = alive.back()->b;
      }
    }
    store->Submit(bs, job, cnt);
    if (pipe) {  // this Submit ran the step before
      MarkAll(&queued);
      queued.swap(now);
    } else {
      MarkAll(&now);
    }
  }
  void Flush() override {
    store->Flush();
    MarkAll(&queued);
  }
};

struct SplitDriver : Driver {
  std::shared_ptr<GpuSplitLearner> sl;
  SplitDriver(const KWArgs& kw, bool pipe) {
    KWArgs k = kw;
    k.push_back({"pipelined", pipe ? "1" : "0"});
    sl = GpuSplitLearner::CreateLoopback(N, k);
  }
  dfx_ctx* ctx(int l) override { return sl->shard(l); }
  void Step(const std::vector<Src>& src, int job, bool cnt) override {
    std::vector<dmlc::RowBlock<feaid_t>> blk(N);
    std::vector<GpuSplitLearner::Item> it(N);
    for (int l = 0; l < N; ++l) {
      if (src[l].dev) {
        it[l].dev = src[l].dev;
        DeviceTextFeed* const feed = src[l].feed;
        const uint64_t ticket = src[l].ticket;
        it[l].release = [feed, ticket]() { feed->Mark(ticket); };
      } else if (src[l].host) {
        blk[l] = src[l].host->GetBlock();
        it[l].host = &blk[l];
      }
    }
    sl->ProcessDeviceBatches(it, job, cnt);
  }
  void Flush() override { sl->Flush(); }
};

struct Result {
  std::vector<std::vector<double>> progress;  // per shard: train {n, loss, auc}, val {..}
  std::vector<std::string> model;             // per shard: the saved file
  size_t steps = 0, unmarked = 0;
};

static std::string Slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static Result Run(bool split, bool pipe, bool device, const std::string& path,
                  const std::string& fmt, const std::string& out_prefix) {
  const std::string keys = fmt == "libsvm" ? "65536" : "262144";
  const KWArgs kw = {{"V_dim", "4"}, {"V_threshold", "1"}, {"lr", "0.1"}, {"V_lr", "0.05"},
                     {"l1", "0.1"}, {"seed", "7"}, {"max_keys", keys}, {"push_agg", "sum"}};
  std::string kws;
  for (const auto& p : kw) kws += (kws.empty() ? "" : ",") + p.first + "=" + p.second;
  std::unique_ptr<Driver> drv;
  if (split)
    drv.reset(new SplitDriver(kw, pipe));
  else
    drv.reset(new A2aDriver(kws, pipe));
  Result out;
  out.progress.resize(N);
  {
    std::vector<std::unique_ptr<DeviceTextFeed>> feeds;
    for (int l = 0; device && l < N; ++l)
      feeds.emplace_back(new DeviceTextFeed(drv->ctx(l), kBatch, kShuf, fmt, kDepth, kDepth));
    for (int train = 1; train >= 0; --train) {
      const int job_type = train ? DFX_JOB_TRAINING : DFX_JOB_VALIDATION;
      for (int job = 0; job < kJobs; ++job) {
        std::vector<std::unique_ptr<BatchReader>> hb(N);
        std::vector<std::unique_ptr<TextReader>> ht(N);
        std::vector<std::unique_ptr<DeviceBatchReader>> dr(N);
        for (int l = 0; l < N; ++l) {
          const int part = job * N + l, nparts = kJobs * N;
          if (device)
            dr[l].reset(new DeviceBatchReader(feeds[l].get(), path, fmt, part, nparts,
                                              train ? kBatch : 0, train ? kShuf : 0,
                                              train ? kNeg : 1.f, 2, kChunk));
          else if (train)
            hb[l].reset(new BatchReader(path, fmt, part, nparts, kBatch, kShuf, kNeg, 2, kChunk));
          else
            ht[l].reset(new TextReader(path, fmt, part, nparts, kChunk, 2));
        }
        std::vector<bool> more(N, true);
        for (;;) {
          bool any = false;
          std::vector<Src> src(N);
          for (int l = 0; l < N; ++l) {
            if (!more[l]) continue;
            if (dr[l]) {
              more[l] = dr[l]->Next();
            } else if (hb[l]) {
              more[l] = hb[l]->Next();
            } else {
              do more[l] = ht[l]->Next();
              while (more[l] && ht[l]->Value().Size() == 0);
            }
            if (!more[l]) continue;
            any = true;
            if (dr[l]) {
              src[l].dev = &dr[l]->Value();
              src[l].feed = feeds[l].get();
              src[l].ticket = dr[l]->Ticket();
            } else {
              src[l].host = hb[l] ? &hb[l]->Value() : &ht[l]->Value();
            }
          }
          if (!any) break;
          drv->Step(src, job_type, train && out.steps < 2);
          ++out.steps;
        }
        // the readers go here, with the job's last batches queued and unmarked (pipelined)
      }
      drv->Flush();
      for (int l = 0; l < N; ++l) {
        dfx_progress p;
        DfxCheck(dfx_progress_read(drv->ctx(l), &p, 1), "dfx_progress_read");
        out.progress[l].insert(out.progress[l].end(), {p.nrows, p.loss, p.auc});
      }
    }
    for (auto& f : feeds) out.unmarked += (size_t)f->Unmarked();
    for (int l = 0; l < N; ++l) {
      DfxCheck(dfx_sync(drv->ctx(l)), "dfx_sync");
      const std::string name = out_prefix + "_part-" + std::to_string(l);
      DfxCheck(dfx_store_save(drv->ctx(l), name.c_str(), 1), "dfx_store_save");
      out.model.push_back(Slurp(name));
    }
    // the feeds go before the contexts
  }
  drv.reset();
  return out;
}

// a model file saved with aux words (dfx_store_save) as key -> the entry's bytes: the file lists
// the table's slots in order, and which slot a key takes is not part of the contract (two runs
// of one command may differ there), so the entries are compared by key — every byte of each
static bool Records(const std::string& raw, std::map<uint64_t, std::string>* out) {
  out->clear();
  if (raw.empty() || raw[0] != 1) return false;
  size_t at = 1;
  while (at < raw.size()) {
    if (at + 12 > raw.size()) return false;
    uint64_t key;
    int size;
    std::memcpy(&key, raw.data() + at, 8);
    std::memcpy(&size, raw.data() + at + 8, 4);
    const size_t n = 24 + (size_t)8 * (size_t)(size - 1);
    if (size < 1 || at + n > raw.size() || out->count(key)) return false;
    (*out)[key] = raw.substr(at + 8, n - 8);
    at += n;
  }
  return !out->empty();
}

static bool SameModels(const Result& a, const Result& b) {
  bool same = a.model.size() == b.model.size() && !a.model.empty();
  for (size_t l = 0; same && l < a.model.size(); ++l) {
    std::map<uint64_t, std::string> ra, rb;
    same = Records(a.model[l], &ra) && Records(b.model[l], &rb) && ra == rb &&
           a.model[l].size() == b.model[l].size();
  }
  return same;
}

static bool SameProgress(const Result& a, const Result& b) {
  bool same = a.progress.size() == b.progress.size();
  for (size_t l = 0; same && l < a.progress.size(); ++l)
    same = a.progress[l].size() == b.progress[l].size() &&
           !std::memcmp(a.progress[l].data(), b.progress[l].data(), a.progress[l].size() * 8);
  return same;
}

// hand-outs with no mark: the reader must throw before it reuses anything
static bool OmittedMarkThrows(const std::string& path, bool whole_chunks, int* handed) {
  dfx_ctx* c = nullptr;
  DfxCheck(dfx_ctx_create(0, "V_dim=4,max_keys=65536", &c), "dfx_ctx_create");
  bool threw = false;
  *handed = 0;
  {
    DeviceTextFeed feed(c, kBatch, kShuf, "libsvm", kDepth, kDepth);
    try {
      DeviceBatchReader r(&feed, path, "libsvm", 0, 1, whole_chunks ? 0 : kBatch,
                          whole_chunks ? 0 : kShuf, 1.f, 2, kChunk);
      while (*handed < 64 && r.Next()) ++*handed;  // no Consumed(), no Mark
    } catch (const FeedProtocolError& e) {
      threw = std::strstr(e.what(), "never marked") != nullptr;
    }
  }
  dfx_ctx_destroy(c);
  return threw;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s rcv1_100.libsvm criteo.txt <scratch dir>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[3];
  const struct {
    const char *name, *path, *fmt;
    double rows;
  } data[2] = {{"rcv1", argv[1], "libsvm", 100}, {"criteo", argv[2], "criteo", 500}};
  for (const auto& d : data) {
    for (int split = 0; split < 2; ++split) {
      for (int pipe = 0; pipe < 2; ++pipe) {
        const std::string name = std::string("data=") + d.name + " store=" +
                                 (split ? "split" : "a2a") + " pipe=" + std::to_string(pipe);
        const Result host = Run(split, pipe, false, d.path, d.fmt, dir + "/h");
        const Result dev = Run(split, pipe, true, d.path, d.fmt, dir + "/d");
        double val_rows = 0, train_rows = 0;
        for (const auto& p : host.progress) {
          train_rows += p[0];
          val_rows += p[3];
        }
        // (training is down-sampled; validation sees every row)
        Report(name, "(the host run stepped: every row validated, some trained)",
               val_rows == d.rows && train_rows > 0 && train_rows <= d.rows && host.steps > 8);
        Report(name, "steps", host.steps == dev.steps);
        Report(name, "progress", SameProgress(host, dev));
        Report(name, "models", SameModels(host, dev));
        Report(name, "(every batch marked after the flush)", dev.unmarked == 0);
      }
    }
  }
  int handed = 0;
  bool threw = OmittedMarkThrows(argv[1], false, &handed);
  std::printf("omitted marks, minibatches: %d handed out, %s\n", handed,
              threw ? "threw" : "NO THROW");
  if (!threw || handed != kDepth) ++g_fail;
  threw = OmittedMarkThrows(argv[1], true, &handed);
  std::printf("omitted marks, whole chunks: %d handed out, %s\n", handed,
              threw ? "threw" : "NO THROW");
  if (!threw || handed != kDepth - 1) ++g_fail;
  std::printf(g_fail ? "FAILED (%d)\n" : "ALL PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
