// train_options_resample_tests.cc — epoch_resample's rows of dfx_train's option rules (CPU only,
// no library; train_options_tests.cc holds the table of every other option): the key parses, the
// two refusals carry their texts, both stand behind every rule of epoch_shuffle and before
// cache=device's, and an accepted run has plan.epoch_resample set.
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../difacto_amd/host/train_options.h"

using namespace difacto;

namespace {
int failures = 0;

struct Resolved {
  int rc;
  std::string err;
  RunPlan plan;
  size_t rest;  // keys Param did not know
};

Resolved Resolve(const std::string& args) {
  std::vector<std::string> words{"dfx_train", "data_in=x"};
  std::istringstream in(args);
  for (std::string w; in >> w;) words.push_back(w);
  std::vector<const char*> argv;
  for (const auto& w : words) argv.push_back(w.c_str());
  Param P;
  KWArgs rest;
  Resolved r;
  r.rc = ParseArgs((int)argv.size(), argv.data(), &P, &rest, &r.err);
  r.rest = rest.size();
  if (r.rc != 0) return r;
  std::vector<std::string> lines;
  r.rc = ResolveOptions(P, rest, LaunchEnv(), &r.plan, &lines, &r.err);
  return r;
}

void Refused(const char* args, const char* err) {
  const Resolved r = Resolve(args);
  if (r.rc != 2 || r.err != err) {
    ++failures;
    std::printf("FAILED [%s]: rc %d, '%s', expected 2, '%s'\n", args, r.rc, r.err.c_str(), err);
  }
}

#define NEEDS_SHUFFLE \
  "epoch_resample=1 needs epoch_shuffle=1 (the rows are drawn out of the reshuffled cache)"
#define NEEDS_SAMPLING "epoch_resample=1 needs neg_sampling < 1"
}  // namespace

int main() {
  // the two refusals, and their order
  Refused("epoch_resample=1", NEEDS_SHUFFLE);
  Refused("epoch_resample=1 cache=device neg_sampling=0.5", NEEDS_SHUFFLE);
  Refused("epoch_resample=1 neg_sampling=1", NEEDS_SHUFFLE);
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device", NEEDS_SAMPLING);
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device neg_sampling=1", NEEDS_SAMPLING);
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device neg_sampling=1.5", NEEDS_SAMPLING);
  // behind every rule of epoch_shuffle, cache_loc and the cache value
  Refused("epoch_resample=1 epoch_shuffle=1",
          "epoch_shuffle=1 needs cache=device (the rows are reshuffled out of the cached batches)");
  Refused("epoch_resample=1 epoch_shuffle=1 cache=auto neg_sampling=0.5",
          "epoch_shuffle=1 needs cache=device (the rows are reshuffled out of the cached batches)");
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device cache_loc=1 neg_sampling=0.5",
          "epoch_shuffle=1 needs cache_loc=0 (reshuffled batches have no kept Localizer outputs)");
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device fused=0",
          "epoch_shuffle=1 needs the fused path (fused=1)");
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device task=2 model_in=m data_val=v",
          "epoch_shuffle=1 needs a training run (task=2 is one pass: nothing is replayed)");
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device shards=2",
          "epoch_shuffle=1 needs the single-GPU run (shards=0)");
  Refused("epoch_resample=1 cache=bogus", "cache must be none, device or auto");
  Refused("epoch_resample=1 cache_loc=1", "cache_loc=1 needs cache=device (the outputs are kept "
                                          "with the cached batches)");
  // ... and before cache=device's own and everything later
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device cache_mb=-1", NEEDS_SAMPLING);
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device pred_write=bogus", NEEDS_SAMPLING);
  Refused("epoch_resample=1 epoch_shuffle=1 cache=device neg_sampling=0.5 cache_mb=-1",
          "cache=device needs cache_mb >= 0");

  // accepted
  Resolved r = Resolve("epoch_resample=1 epoch_shuffle=1 cache=device neg_sampling=0.5");
  if (r.rc != 0 || !r.plan.epoch_resample || !r.plan.epoch_shuffle || !r.plan.cache || r.rest) {
    ++failures;
    std::printf("FAILED: the accepted run: rc %d '%s' resample %d, %zu unknown keys\n", r.rc,
                r.err.c_str(), (int)r.plan.epoch_resample, r.rest);
  }
  // off: by default, with epoch_resample=0, and with epoch_shuffle=1 alone
  for (const char* args : {"", "epoch_resample=0", "epoch_resample=0 neg_sampling=0.5",
                           "epoch_shuffle=1 cache=device neg_sampling=0.5"}) {
    r = Resolve(args);
    if (r.rc != 0 || r.plan.epoch_resample || r.rest) {
      ++failures;
      std::printf("FAILED [%s]: rc %d '%s' resample %d, %zu unknown keys\n", args, r.rc,
                  r.err.c_str(), (int)r.plan.epoch_resample, r.rest);
    }
  }
  if (RunPlan().epoch_resample || Param().epoch_resample) {
    ++failures;
    std::printf("FAILED: epoch_resample is not off by default\n");
  }
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("train_options_resample_tests: all passed\n");
  return 0;
}
