// train_options.h — dfx_train's command line (train_main.cc's head comment describes the
// options) and its one resolution step: Param is what the user wrote, LaunchEnv what the
// launcher set, RunPlan what the run will do.  ResolveOptions holds every refusal rule and every
// "which path and why" line, in the order that decides which message wins; the run loops read
// the plan and never compare an option's string again.  No HIP and no adapter header: plain
// g++ builds it alone (tests/host/train_options_tests.cc is its truth table).
#ifndef DIFACTO_AMD_HOST_TRAIN_OPTIONS_H_
#define DIFACTO_AMD_HOST_TRAIN_OPTIONS_H_

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "iface.h"  // KWArgs

namespace difacto {

struct Param {
  std::string data_in, data_val, data_format = "libsvm", model_in, model_out, pred_out;
  size_t batch_size = 100, shuffle = 10;
  float neg_sampling = 1.f;
  int max_num_epochs = 20, num_jobs_per_epoch = 10, nthreads = 8;
  int load_epoch = -1, task = 0;
  int shards = 0;  // > 0: that many loopback shards in this process; -1: one shard, RCCL
  int model_in_parts = 0;  // servers that saved model_in, when not this run's shard count
  bool pipelined = true;
  std::string exchange = "a2a";  // a2a: GpuShardedStore (KVStoreDist); split: GpuSplitLearner
  bool has_aux = false, pred_prob = true;
  double stop_rel_objv = 1e-5;
  double stop_val_auc = 1e-5;  // sgd_param.h:73
  std::string parse = "host";  // host|device|auto|auto-sharded
  bool parse_adfea = false;    // adfea has a device parser too (under auto, auto-sharded)
  std::string cache = "none";  // none|device|auto
  int64_t cache_mb = 16384;    // its budget (per shard)
  bool cache_loc = false;      // the Localizer's outputs kept with the cached batches too
  bool epoch_shuffle = false;  // replayed training parts are reshuffled on the device per epoch
  uint64_t shuffle_seed = 0;   // ... keyed by (shuffle_seed, epoch, list)
  bool epoch_resample = false;  // ... and negatives are down-sampled afresh per epoch there
  std::string pred_write = "host";  // host|device
  std::string model_write = "host";  // host|device: who lays down model_out / name_dump
  // task=1 (src/reader/dump.h): model_in, the literal file, as text into name_dump
  std::string name_dump = "dump.txt";
  bool need_reverse = false, dump_aux = false;
};

/** argv into P; a key Param does not know goes to rest (the context's and the updater's).
 * 0, or 2 with the message in err */
inline int ParseArgs(int argc, const char* const* argv, Param* Pp, KWArgs* rest,
                     std::string* err) {
  Param& P = *Pp;
  for (int i = 1; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    if (!eq) {
      *err = std::string("argument '") + argv[i] + "' is not key=value";
      return 2;
    }
    const std::string k(argv[i], eq - argv[i]), v(eq + 1);
    if (k == "data_in") P.data_in = v;
    else if (k == "data_val") P.data_val = v;
    else if (k == "data_format") P.data_format = v;
    else if (k == "model_in") P.model_in = v;
    else if (k == "model_out") P.model_out = v;
    else if (k == "batch_size") P.batch_size = std::stoul(v);
    else if (k == "shuffle") P.shuffle = std::stoul(v);
    else if (k == "neg_sampling") P.neg_sampling = std::stof(v);
    else if (k == "max_num_epochs") P.max_num_epochs = std::stoi(v);
    else if (k == "num_jobs_per_epoch") P.num_jobs_per_epoch = std::stoi(v);
    else if (k == "stop_rel_objv") P.stop_rel_objv = std::stod(v);
    else if (k == "stop_val_auc") P.stop_val_auc = std::stod(v);
    else if (k == "nthreads") P.nthreads = std::stoi(v);
    else if (k == "load_epoch") P.load_epoch = std::stoi(v);
    else if (k == "task") P.task = std::stoi(v);
    else if (k == "pred_out") P.pred_out = v;
    else if (k == "pred_prob") P.pred_prob = std::stoi(v) != 0;
    else if (k == "has_aux") P.has_aux = std::stoi(v) != 0;
    else if (k == "shards") P.shards = std::stoi(v);
    else if (k == "pipelined") P.pipelined = std::stoi(v) != 0;
    else if (k == "exchange") P.exchange = v;
    else if (k == "model_in_parts") P.model_in_parts = std::stoi(v);
    else if (k == "parse") P.parse = v;
    else if (k == "parse_adfea") P.parse_adfea = std::stoi(v) != 0;
    else if (k == "cache") P.cache = v;
    else if (k == "cache_mb") P.cache_mb = std::stoll(v);
    else if (k == "cache_loc") P.cache_loc = std::stoi(v) != 0;
    else if (k == "epoch_shuffle") P.epoch_shuffle = std::stoi(v) != 0;
    else if (k == "shuffle_seed") P.shuffle_seed = std::stoull(v);
    else if (k == "epoch_resample") P.epoch_resample = std::stoi(v) != 0;
    else if (k == "pred_write") P.pred_write = v;
    else if (k == "model_write") P.model_write = v;
    else if (k == "name_dump") P.name_dump = v;
    else if (k == "need_reverse") P.need_reverse = std::stoi(v) != 0;
    else if (k == "dump_aux") P.dump_aux = std::stoi(v) != 0;
    else rest->push_back({k, v});
  }
  if (P.data_in.empty() && P.task != 2 && P.task != 1) {
    *err = std::string("usage: ") + argv[0] + " data_in=FILE [key=value ...]";
    return 2;
  }
  return 0;
}

/** what the launcher set (torchrun's names); a test constructs one directly */
struct LaunchEnv {
  int world = 1, rank = 0, local_rank = 0;
  std::string comm_id_file;  // the node-local RCCL rendezvous
  static LaunchEnv FromEnvironment() {
    const auto num = [](const char* s, int dflt) { return s ? std::atoi(s) : dflt; };
    LaunchEnv e;
    e.world = num(std::getenv("WORLD_SIZE"), 1);
    e.rank = num(std::getenv("RANK"), 0);
    e.local_rank = num(std::getenv("LOCAL_RANK"), 0);
    if (const char* f = std::getenv("DFX_COMM_ID_FILE")) {
      e.comm_id_file = f;
    } else {
      const char* port = std::getenv("MASTER_PORT");
      e.comm_id_file = std::string("/tmp/dfx_comm_") + (port ? port : "0");
    }
    return e;
  }
};

struct RunPlan {
  bool sharded = false;  // shards != 0 or WORLD_SIZE > 1: RunSharded
  bool rccl = false;     // one shard per process over RCCL, else loopback shards
  int nshards = 1;       // as the parse: line names them
  bool fused = true, fused_given = false;  // the last fused= of rest
  enum class Parse { kHost, kDevice };
  Parse parse = Parse::kHost;  // kDevice: a DeviceTextFeed is made (per shard in a sharded run)
  bool cache = false;          // a DeviceBatchCache is made (never with task=2: one pass)
  bool cache_loc = false, epoch_shuffle = false;
  bool epoch_resample = false;  // every training epoch draws its negatives out of the full cache
  bool pred_write_device = false;
  bool model_write_device = false;  // model_out / name_dump through the device writers
  bool dump = false;                // task=1: load model_in, write name_dump, nothing else
  bool print_rank = true;  // rank 0, or an unsharded run: prints the run's lines
};

/** Every option rule of dfx_train, in the order that decides which refusal wins: the parse
 * value, parse_adfea (the format, then the parse value), auto-sharded, auto, device; the cache
 * value, cache_loc, epoch_shuffle, epoch_resample, cache=device, cache=auto; the pred_write
 * value, pred_write=device; the prediction inputs; exchange; the model_write value; task=1's
 * inputs.  The lines resolved before a
 * refusal stay in out_lines (main prints them first).  0, or 2 with the message in err.  Prints
 * nothing and reads no environment. */
inline int ResolveOptions(const Param& P, const KWArgs& rest, const LaunchEnv& env, RunPlan* plan,
                          std::vector<std::string>* out_lines, std::string* err) {
  RunPlan& R = *plan;
  R = RunPlan();
  for (const auto& kv : rest)
    if (kv.first == "fused") {
      R.fused_given = true;
      R.fused = std::stoi(kv.second) != 0;
    }
  R.sharded = P.shards != 0 || env.world > 1;
  R.rccl = env.world > 1 || P.shards < 0;
  R.nshards = P.shards > 0 ? P.shards : env.world > 1 ? env.world : 1;
  R.print_rank = !R.sharded || env.rank == 0;
  const bool sharded = R.sharded, fused = R.fused;
  const auto refuse = [err](const std::string& what, const char* why) {
    *err = what + why;
    return 2;
  };
  const bool criteo = P.data_format == "criteo" || P.data_format == "criteo_test";
  const bool dev_parser = criteo || P.data_format == "libsvm" ||
                          (P.parse_adfea && P.data_format == "adfea");

  if (P.parse != "host" && P.parse != "device" && P.parse != "auto" && P.parse != "auto-sharded")
    return refuse("parse must be host, device, auto or auto-sharded", "");
  if (P.parse_adfea) {  // no silent run on the host reader
    const char* const what = "parse_adfea=1 needs ";
    if (P.data_format != "adfea") return refuse(what, "data_format=adfea");
    if (P.parse != "auto" && P.parse != "auto-sharded")
      return refuse(what, "parse=auto or parse=auto-sharded");
  }
  if (P.parse == "auto-sharded" && sharded) {
    // the device parser in the sharded run too, where the format has one
    if (R.print_rank)
      out_lines->push_back(dev_parser ? "parse: device (" + P.data_format + ", " +
                                            std::to_string(R.nshards) + " shards)"
                                      : "parse: host (data_format=" + P.data_format + ")");
    if (dev_parser) R.parse = RunPlan::Parse::kDevice;
  } else if (P.parse == "auto" || P.parse == "auto-sharded") {
    // the device parser where there is one, and a line saying which (every rank prints it)
    std::string why;
    if (sharded)
      why = P.exchange == "split" ? "exchange=split" : "a sharded run";
    else if (!fused)
      why = "fused=0";
    else if (!dev_parser)
      why = "data_format=" + P.data_format;
    out_lines->push_back(why.empty() ? "parse: device (" + P.data_format + ")"
                                     : "parse: host (" + why + ")");
    if (why.empty()) R.parse = RunPlan::Parse::kDevice;
  } else if (P.parse == "device") {  // no silent fall-back to the host reader
    if (!criteo) return refuse("parse=device needs ", "data_format=criteo or criteo_test");
    if (!fused) return refuse("parse=device needs ", "the fused path (fused=1)");
    if (sharded) return refuse("parse=device needs ", "the single-GPU run (shards=0)");
    R.parse = RunPlan::Parse::kDevice;
  }

  if (P.cache != "none" && P.cache != "device" && P.cache != "auto")
    return refuse("cache must be none, device or auto", "");
  if (P.cache_loc) {  // no silent run without the kept outputs
    const char* const what = "cache_loc=1 needs ";
    if (P.cache != "device")
      return refuse(what, "cache=device (the outputs are kept with the cached batches)");
    if (!fused) return refuse(what, "the fused path (fused=1)");
    if (P.task == 2)
      return refuse(what, "a training run (task=2 is one pass: nothing is replayed)");
    if (sharded)
      return refuse(what, "the single-GPU run (shards=0): the sharded paths localize per shard");
  }
  if (P.epoch_shuffle) {  // no silent run in the recorded order
    const char* const what = "epoch_shuffle=1 needs ";
    if (P.cache != "device")
      return refuse(what, "cache=device (the rows are reshuffled out of the cached batches)");
    if (P.cache_loc)
      return refuse(what, "cache_loc=0 (reshuffled batches have no kept Localizer outputs)");
    if (!fused) return refuse(what, "the fused path (fused=1)");
    if (P.task == 2)
      return refuse(what, "a training run (task=2 is one pass: nothing is replayed)");
    if (sharded) return refuse(what, "the single-GPU run (shards=0)");
  }
  if (P.epoch_resample) {  // no silent run on the reader's one sample
    const char* const what = "epoch_resample=1 needs ";
    if (!P.epoch_shuffle)
      return refuse(what, "epoch_shuffle=1 (the rows are drawn out of the reshuffled cache)");
    if (!(P.neg_sampling < 1.f)) return refuse(what, "neg_sampling < 1");
  }
  R.cache_loc = P.cache_loc;
  R.epoch_shuffle = P.epoch_shuffle;
  R.epoch_resample = P.epoch_resample;
  if (P.cache == "device") {  // no silent run without the cache
    const char* const what = "cache=device needs ";
    if (!fused) return refuse(what, "the fused path (fused=1)");
    if (sharded && P.exchange == "split")
      return refuse(what, "exchange=a2a in a sharded run (exchange=split replays under "
                          "cache=auto)");
    if (P.cache_mb < 0) return refuse(what, "cache_mb >= 0");
    R.cache = P.task != 2;  // accepted with task=2, where it has no effect
  } else if (P.cache == "auto") {
    // the device cache where batches replay, and a line saying which; a sharded run replays
    // whatever fused says
    if (P.cache_mb < 0) return refuse("cache=auto needs ", "cache_mb >= 0");
    R.cache = (sharded || fused) && P.task != 2;
    const std::string why = !sharded && !fused ? "fused=0"
                            : P.task == 2      ? "task=2"
                            : sharded          ? "exchange=" + P.exchange
                                               : "fused";
    if (R.print_rank)
      out_lines->push_back(std::string("cache: ") + (R.cache ? "device" : "none") + " (" + why +
                           ")");
  }

  if (P.pred_write != "host" && P.pred_write != "device")
    return refuse("pred_write must be host or device", "");
  R.pred_write_device = P.pred_write == "device";
  if (R.pred_write_device && !fused)  // no silent fall-back to the host writer
    return refuse("pred_write=device needs ", "the fused path (fused=1): the interface path "
                                              "keeps its predictions on the host");
  if (P.task == 2 && (P.model_in.empty() || P.data_val.empty()))
    return refuse("prediction needs model_in and data_val", "");
  if (sharded && P.exchange != "a2a" && P.exchange != "split")
    return refuse("exchange must be a2a or split", "");
  if (P.model_write != "host" && P.model_write != "device")
    return refuse("model_write must be host or device", "");
  R.model_write_device = P.model_write == "device";  // (without model_out: nothing to write)
  R.dump = P.task == 1;
  if (R.dump) {
    if (P.model_in.empty()) return refuse("dump needs model_in", "");
    if (sharded) return refuse("task=1 needs ", "the single-GPU run (shards=0)");
  }
  return 0;
}

}  // namespace difacto
#endif  // DIFACTO_AMD_HOST_TRAIN_OPTIONS_H_
