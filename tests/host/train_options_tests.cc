// train_options_tests.cc — the truth table of dfx_train's option rules (CPU only, no library):
// ParseArgs + ResolveOptions (difacto_amd/host/train_options.h) on rows of (arguments, launch
// environment) against the exit status, the stderr message, the stdout lines and the RunPlan.
// The order of the table is the order of the checks, which decides which refusal wins and
// which lines are already out when a later option is refused.
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../difacto_amd/host/train_options.h"

using namespace difacto;

namespace {
int failures = 0;

#define EXPECT(cond, what)                                                     \
  do {                                                                         \
    if (!(cond)) {                                                             \
      ++failures;                                                              \
      std::printf("FAILED %s:%d: [%s] %s\n", __FILE__, __LINE__, what, #cond); \
    }                                                                          \
  } while (0)

struct Resolved {
  int rc;
  std::string err, lines;  // the lines joined, each with its '\n'
  RunPlan plan;
};

// "data_in=x" + the row's arguments, through ParseArgs and (if it accepts) ResolveOptions
Resolved Resolve(const std::string& args, int world = 1, int rank = 0, bool data_in = true) {
  std::vector<std::string> words{"dfx_train"};
  if (data_in) words.push_back("data_in=x");
  std::istringstream in(args);
  for (std::string w; in >> w;) words.push_back(w);
  std::vector<const char*> argv;
  for (const auto& w : words) argv.push_back(w.c_str());
  Param P;
  KWArgs rest;
  Resolved r;
  r.rc = ParseArgs((int)argv.size(), argv.data(), &P, &rest, &r.err);
  if (r.rc != 0) return r;
  LaunchEnv env;
  env.world = world;
  env.rank = rank;
  std::vector<std::string> lines;
  r.rc = ResolveOptions(P, rest, env, &r.plan, &lines, &r.err);
  for (const auto& l : lines) r.lines += l + "\n";
  return r;
}

const int kAny = -1, kHost = 0, kDev = 1;

struct Row {
  const char* args;
  int world, rank;
  int rc;
  const char* err;    // the whole message
  const char* lines;  // the whole stdout
  int parse, cache;   // the plan's (kAny: a refused row)
};

#define NEEDS_FUSED "the fused path (fused=1)"
#define ONE_PASS "a training run (task=2 is one pass: nothing is replayed)"
#define PRED_IN "model_in=m data_val=v"

const Row kRows[] = {
    // ---- 1. the parse value
    {"parse=bogus", 1, 0, 2, "parse must be host, device, auto or auto-sharded", "", kAny, kAny},
    {"", 1, 0, 0, "", "", kHost, 0},
    {"parse=host shards=2", 1, 0, 0, "", "", kHost, 0},
    // ---- 2. auto-sharded: parse=auto without shards, else the device parser per shard
    {"parse=auto-sharded", 1, 0, 0, "", "parse: device (libsvm)\n", kDev, 0},
    {"parse=auto-sharded fused=0", 1, 0, 0, "", "parse: host (fused=0)\n", kHost, 0},
    {"parse=auto-sharded shards=2", 1, 0, 0, "", "parse: device (libsvm, 2 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=2 exchange=split data_format=criteo", 1, 0, 0, "",
     "parse: device (criteo, 2 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=2 fused=0 data_format=criteo_test", 1, 0, 0, "",
     "parse: device (criteo_test, 2 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=-1", 4, 0, 0, "", "parse: device (libsvm, 4 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=-1", 4, 1, 0, "", "", kDev, 0},
    {"parse=auto-sharded", 2, 0, 0, "", "parse: device (libsvm, 2 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=-1", 1, 0, 0, "", "parse: device (libsvm, 1 shards)\n", kDev, 0},
    {"parse=auto-sharded shards=2 data_format=rec", 1, 0, 0, "", "parse: host (data_format=rec)\n",
     kHost, 0},
    {"parse=auto-sharded shards=2 data_format=rec", 2, 1, 0, "", "", kHost, 0},
    // ---- 3. auto (its line is printed by every rank)
    {"parse=auto", 1, 0, 0, "", "parse: device (libsvm)\n", kDev, 0},
    {"parse=auto data_format=criteo", 1, 0, 0, "", "parse: device (criteo)\n", kDev, 0},
    {"parse=auto data_format=criteo_test", 1, 3, 0, "", "parse: device (criteo_test)\n", kDev, 0},
    {"parse=auto shards=2 exchange=split", 1, 0, 0, "", "parse: host (exchange=split)\n", kHost, 0},
    {"parse=auto shards=2", 1, 0, 0, "", "parse: host (a sharded run)\n", kHost, 0},
    {"parse=auto", 2, 1, 0, "", "parse: host (a sharded run)\n", kHost, 0},
    {"parse=auto shards=2 fused=0 data_format=rec", 1, 0, 0, "", "parse: host (a sharded run)\n",
     kHost, 0},
    {"parse=auto fused=0", 1, 0, 0, "", "parse: host (fused=0)\n", kHost, 0},
    {"parse=auto fused=0 data_format=rec", 1, 0, 0, "", "parse: host (fused=0)\n", kHost, 0},
    {"parse=auto data_format=rec", 1, 0, 0, "", "parse: host (data_format=rec)\n", kHost, 0},
    // ---- 4. device: format, then fused, then sharded
    {"parse=device", 1, 0, 2, "parse=device needs data_format=criteo or criteo_test", "", kAny,
     kAny},
    {"parse=device fused=0 shards=2", 1, 0, 2,
     "parse=device needs data_format=criteo or criteo_test", "", kAny, kAny},
    {"parse=device data_format=criteo fused=0 shards=2", 1, 0, 2,
     "parse=device needs " NEEDS_FUSED, "", kAny, kAny},
    {"parse=device data_format=criteo_test shards=2", 1, 0, 2,
     "parse=device needs the single-GPU run (shards=0)", "", kAny, kAny},
    {"parse=device data_format=criteo", 2, 0, 2,
     "parse=device needs the single-GPU run (shards=0)", "", kAny, kAny},
    {"parse=device data_format=criteo", 1, 0, 0, "", "", kDev, 0},
    {"parse=device data_format=criteo_test", 1, 0, 0, "", "", kDev, 0},
    // ---- 5. the cache value (the parse line is already out)
    {"cache=bogus", 1, 0, 2, "cache must be none, device or auto", "", kAny, kAny},
    {"parse=auto cache=bogus", 1, 0, 2, "cache must be none, device or auto",
     "parse: device (libsvm)\n", kAny, kAny},
    // ---- 6. cache_loc: cache=device literally, fused, not task=2, not sharded
    {"cache_loc=1", 1, 0, 2,
     "cache_loc=1 needs cache=device (the outputs are kept with the cached batches)", "", kAny,
     kAny},
    {"cache_loc=1 cache=auto fused=0 task=2 shards=2", 1, 0, 2,
     "cache_loc=1 needs cache=device (the outputs are kept with the cached batches)", "", kAny,
     kAny},
    {"cache_loc=1 cache=device fused=0 task=2 shards=2", 1, 0, 2,
     "cache_loc=1 needs " NEEDS_FUSED, "", kAny, kAny},
    {"cache_loc=1 cache=device task=2 shards=2", 1, 0, 2, "cache_loc=1 needs " ONE_PASS, "", kAny,
     kAny},
    {"cache_loc=1 cache=device shards=2", 1, 0, 2,
     "cache_loc=1 needs the single-GPU run (shards=0): the sharded paths localize per shard", "",
     kAny, kAny},
    {"cache_loc=1 cache=device", 1, 0, 0, "", "", kHost, 1},
    // ---- 7. epoch_shuffle: cache=device literally, not cache_loc, fused, not task=2, not sharded
    {"epoch_shuffle=1", 1, 0, 2,
     "epoch_shuffle=1 needs cache=device (the rows are reshuffled out of the cached batches)", "",
     kAny, kAny},
    {"epoch_shuffle=1 cache=auto", 1, 0, 2,
     "epoch_shuffle=1 needs cache=device (the rows are reshuffled out of the cached batches)", "",
     kAny, kAny},
    {"epoch_shuffle=1 cache=device cache_loc=1", 1, 0, 2,
     "epoch_shuffle=1 needs cache_loc=0 (reshuffled batches have no kept Localizer outputs)", "",
     kAny, kAny},
    {"epoch_shuffle=1 cache_loc=1", 1, 0, 2,  // cache_loc's own check comes first
     "cache_loc=1 needs cache=device (the outputs are kept with the cached batches)", "", kAny,
     kAny},
    {"epoch_shuffle=1 cache=device fused=0 task=2 shards=2", 1, 0, 2,
     "epoch_shuffle=1 needs " NEEDS_FUSED, "", kAny, kAny},
    {"epoch_shuffle=1 cache=device task=2 shards=2", 1, 0, 2, "epoch_shuffle=1 needs " ONE_PASS,
     "", kAny, kAny},
    {"epoch_shuffle=1 cache=device shards=2", 1, 0, 2,
     "epoch_shuffle=1 needs the single-GPU run (shards=0)", "", kAny, kAny},
    {"epoch_shuffle=1 cache=device", 1, 0, 0, "", "", kHost, 1},
    // ---- 8. cache=device: fused (sharded too), exchange=a2a, a budget
    {"cache=device fused=0", 1, 0, 2, "cache=device needs " NEEDS_FUSED, "", kAny, kAny},
    {"cache=device fused=0 shards=2 exchange=split cache_mb=-1", 1, 0, 2,
     "cache=device needs " NEEDS_FUSED, "", kAny, kAny},
    {"cache=device shards=2 exchange=split cache_mb=-1", 1, 0, 2,
     "cache=device needs exchange=a2a in a sharded run (exchange=split replays under cache=auto)",
     "", kAny, kAny},
    {"cache=device cache_mb=-1", 1, 0, 2, "cache=device needs cache_mb >= 0", "", kAny, kAny},
    {"cache=device", 1, 0, 0, "", "", kHost, 1},
    {"cache=device exchange=split", 1, 0, 0, "", "", kHost, 1},  // unsharded: exchange unused
    {"cache=device shards=2", 1, 0, 0, "", "", kHost, 1},
    {"cache=device cache_mb=0", 1, 0, 0, "", "", kHost, 1},
    {"cache=device task=2 " PRED_IN, 1, 0, 0, "", "", kHost, 0},  // accepted, no effect
    {"cache=device task=2 shards=2 " PRED_IN, 1, 0, 0, "", "", kHost, 0},
    // ---- 9. cache=auto: the budget before its line, then which and why
    {"cache=auto cache_mb=-1", 1, 0, 2, "cache=auto needs cache_mb >= 0", "", kAny, kAny},
    {"cache=auto cache_mb=-1 shards=2 exchange=split", 1, 0, 2, "cache=auto needs cache_mb >= 0",
     "", kAny, kAny},
    {"cache=auto cache_mb=-1 shards=2", 1, 0, 2, "cache=auto needs cache_mb >= 0", "", kAny, kAny},
    {"cache=auto cache_mb=-1 fused=0", 1, 0, 2, "cache=auto needs cache_mb >= 0", "", kAny, kAny},
    {"parse=auto cache=auto cache_mb=-1", 1, 0, 2, "cache=auto needs cache_mb >= 0",
     "parse: device (libsvm)\n", kAny, kAny},
    {"cache=auto", 1, 0, 0, "", "cache: device (fused)\n", kHost, 1},
    {"cache=auto", 1, 1, 0, "", "cache: device (fused)\n", kHost, 1},  // unsharded: RANK unused
    {"cache=auto shards=2", 1, 0, 0, "", "cache: device (exchange=a2a)\n", kHost, 1},
    {"cache=auto shards=2 exchange=split", 1, 0, 0, "", "cache: device (exchange=split)\n", kHost,
     1},
    {"cache=auto fused=0", 1, 0, 0, "", "cache: none (fused=0)\n", kHost, 0},
    {"cache=auto task=2 " PRED_IN, 1, 0, 0, "", "cache: none (task=2)\n", kHost, 0},
    {"cache=auto task=2 shards=2 " PRED_IN, 1, 0, 0, "", "cache: none (task=2)\n", kHost, 0},
    {"cache=auto shards=2 fused=0", 1, 0, 0, "", "cache: device (exchange=a2a)\n", kHost, 1},
    {"cache=auto fused=0 task=2 " PRED_IN, 1, 0, 0, "", "cache: none (fused=0)\n", kHost, 0},
    {"cache=auto", 2, 1, 0, "", "", kHost, 1},
    {"cache=auto exchange=split fused=0", 2, 1, 0, "", "", kHost, 1},
    {"cache=auto task=2 " PRED_IN, 2, 1, 0, "", "", kHost, 0},
    {"parse=auto-sharded cache=auto shards=2", 1, 0, 0, "",
     "parse: device (libsvm, 2 shards)\ncache: device (exchange=a2a)\n", kDev, 1},
    // ---- 10, 11. the pred_write value; pred_write=device needs the fused path
    {"pred_write=bogus", 1, 0, 2, "pred_write must be host or device", "", kAny, kAny},
    {"cache=auto pred_write=bogus", 1, 0, 2, "pred_write must be host or device",
     "cache: device (fused)\n", kAny, kAny},
    {"pred_write=device fused=0", 1, 0, 2,
     "pred_write=device needs the fused path (fused=1): the interface path keeps its predictions "
     "on the host",
     "", kAny, kAny},
    {"pred_write=device fused=0 task=2 shards=2", 1, 0, 2,  // before the prediction inputs
     "pred_write=device needs the fused path (fused=1): the interface path keeps its predictions "
     "on the host",
     "", kAny, kAny},
    {"pred_write=device", 1, 0, 0, "", "", kHost, 0},  // without task=2: accepted, does nothing
    {"pred_write=device task=2 shards=2 exchange=split " PRED_IN, 1, 0, 0, "", "", kHost, 0},
    // ---- 12. the prediction inputs, sharded or not
    {"task=2 shards=2", 1, 0, 2, "prediction needs model_in and data_val", "", kAny, kAny},
    {"task=2 shards=2 model_in=m", 1, 0, 2, "prediction needs model_in and data_val", "", kAny,
     kAny},
    {"task=2 data_val=v", 2, 1, 2, "prediction needs model_in and data_val", "", kAny, kAny},
    {"task=2", 1, 0, 2, "prediction needs model_in and data_val", "", kAny, kAny},
    {"task=2 model_in=m", 1, 0, 2, "prediction needs model_in and data_val", "", kAny, kAny},
    {"cache=auto task=2", 1, 0, 2, "prediction needs model_in and data_val",
     "cache: none (task=2)\n", kAny, kAny},
    {"task=2 " PRED_IN, 1, 0, 0, "", "", kHost, 0},
    // ---- 13. exchange, after every other check, in a sharded run only
    {"exchange=bogus shards=2", 1, 0, 2, "exchange must be a2a or split", "", kAny, kAny},
    {"exchange=bogus shards=2 task=2", 1, 0, 2, "prediction needs model_in and data_val", "",
     kAny, kAny},
    {"exchange=bogus shards=2 parse=auto cache=auto", 1, 0, 2, "exchange must be a2a or split",
     "parse: host (a sharded run)\ncache: device (exchange=bogus)\n", kAny, kAny},
    {"exchange=bogus", 1, 0, 0, "", "", kHost, 0},
};

void TestRows() {
  for (const Row& row : kRows) {
    const Resolved r = Resolve(row.args, row.world, row.rank);
    const std::string what = std::string(row.args) + " world=" + std::to_string(row.world) +
                             " rank=" + std::to_string(row.rank);
    EXPECT(r.rc == row.rc, what.c_str());
    EXPECT(r.err == row.err, what.c_str());
    EXPECT(r.lines == row.lines, what.c_str());
    if (r.err != row.err || r.lines != row.lines)
      std::printf("  got err \"%s\" lines \"%s\"\n", r.err.c_str(), r.lines.c_str());
    if (row.parse != kAny)
      EXPECT((r.plan.parse == RunPlan::Parse::kDevice) == (row.parse == kDev), what.c_str());
    if (row.cache != kAny) EXPECT(r.plan.cache == (row.cache != 0), what.c_str());
  }
}

// the plan's other fields
void TestPlanFields() {
  Resolved r = Resolve("");
  EXPECT(!r.plan.sharded && !r.plan.rccl && r.plan.nshards == 1 && r.plan.print_rank, "default");
  EXPECT(r.plan.fused && !r.plan.fused_given, "default");
  EXPECT(!r.plan.cache_loc && !r.plan.epoch_shuffle && !r.plan.pred_write_device, "default");
  r = Resolve("", 1, 3);
  EXPECT(!r.plan.sharded && r.plan.print_rank, "RANK without WORLD_SIZE");
  r = Resolve("shards=2");
  EXPECT(r.plan.sharded && !r.plan.rccl && r.plan.nshards == 2 && r.plan.print_rank, "shards=2");
  r = Resolve("shards=-1");
  EXPECT(r.plan.sharded && r.plan.rccl && r.plan.nshards == 1, "shards=-1");
  r = Resolve("", 4, 3);
  EXPECT(r.plan.sharded && r.plan.rccl && r.plan.nshards == 4 && !r.plan.print_rank, "world=4");
  r = Resolve("shards=-1", 4, 0);
  EXPECT(r.plan.sharded && r.plan.rccl && r.plan.nshards == 4 && r.plan.print_rank, "world=4");
  r = Resolve("fused=0");
  EXPECT(!r.plan.fused && r.plan.fused_given, "fused=0");
  r = Resolve("fused=0 V_dim=4 fused=1");  // the last one counts
  EXPECT(r.plan.fused && r.plan.fused_given, "fused=0 fused=1");
  r = Resolve("cache=device cache_loc=1");
  EXPECT(r.rc == 0 && r.plan.cache_loc && !r.plan.epoch_shuffle, "cache_loc=1");
  r = Resolve("cache=device epoch_shuffle=1");
  EXPECT(r.rc == 0 && !r.plan.cache_loc && r.plan.epoch_shuffle, "epoch_shuffle=1");
  r = Resolve("pred_write=device");
  EXPECT(r.rc == 0 && r.plan.pred_write_device, "pred_write=device");
}

// the command line itself
void TestParseArgs() {
  Resolved r = Resolve("parse", 1, 0);
  EXPECT(r.rc == 2 && r.err == "argument 'parse' is not key=value", "no '='");
  r = Resolve("", 1, 0, false);
  EXPECT(r.rc == 2 && r.err == "usage: dfx_train data_in=FILE [key=value ...]", "no data_in");
  r = Resolve("task=2 " PRED_IN, 1, 0, false);  // a prediction run reads no data_in
  EXPECT(r.rc == 0, "task=2 without data_in");
  const char* argv[] = {"dfx_train", "data_in=a", "batch_size=7", "lr=.1", "cache_mb=-3",
                        "shuffle_seed=18446744073709551615", "pipelined=0", "V_dim=2"};
  Param P;
  KWArgs rest;
  std::string err;
  EXPECT(ParseArgs(8, argv, &P, &rest, &err) == 0, "ParseArgs");
  EXPECT(P.data_in == "a" && P.batch_size == 7 && P.cache_mb == -3 && !P.pipelined, "ParseArgs");
  EXPECT(P.shuffle_seed == 18446744073709551615ull, "ParseArgs");
  EXPECT((rest == KWArgs{{"lr", ".1"}, {"V_dim", "2"}}), "ParseArgs: the unknown keys, in order");
}
}  // namespace

int main() {
  TestRows();
  TestPlanFields();
  TestParseArgs();
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("ALL PASSED (%zu rows)\n", sizeof(kRows) / sizeof(kRows[0]));
  return 0;
}
