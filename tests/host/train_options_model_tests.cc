// train_options_model_tests.cc — model_write's and task=1's rows of dfx_train's option rules (CPU
// only, no library; train_options_tests.cc holds the table of every older option): the
// model_write value rule, task=1 with and without model_in, task=1 in a sharded invocation,
// task=1 passing ParseArgs with no data_in, and both new rules standing behind every older
// refusal; against the exit status, the stderr message and the plan's model_write_device / dump.
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
  bool parsed;  // ParseArgs accepted the line
  std::string err;
  RunPlan plan;
  Param P;
  size_t rest;
};

Resolved Resolve(const std::string& args) {
  std::vector<std::string> words{"dfx_train"};
  std::istringstream in(args);
  for (std::string w; in >> w;) words.push_back(w);
  std::vector<const char*> argv;
  for (const auto& w : words) argv.push_back(w.c_str());
  KWArgs rest;
  Resolved r;
  r.rc = ParseArgs((int)argv.size(), argv.data(), &r.P, &rest, &r.err);
  r.parsed = r.rc == 0;
  r.rest = rest.size();
  if (r.rc != 0) return r;
  std::vector<std::string> lines;
  r.rc = ResolveOptions(r.P, rest, LaunchEnv(), &r.plan, &lines, &r.err);
  return r;
}

const int kAny = -1;

struct Row {
  const char* args;
  int rc;
  const char* err;  // the whole message
  int device;       // the plan's model_write_device (kAny: a refused row)
  int dump;         // ... and dump
};

#define VALUE "model_write must be host or device"
#define NEEDS_IN "dump needs model_in"
#define NEEDS_SINGLE "task=1 needs the single-GPU run (shards=0)"

const Row kRows[] = {
    // ---- model_write: the value rule; accepted on every path, with or without model_out
    {"data_in=x", 0, "", 0, 0},
    {"data_in=x model_write=host", 0, "", 0, 0},
    {"data_in=x model_write=device", 0, "", 1, 0},
    {"data_in=x model_write=device model_out=m", 0, "", 1, 0},
    {"data_in=x model_write=device model_out=m fused=0", 0, "", 1, 0},
    {"data_in=x model_write=device model_out=m shards=2", 0, "", 1, 0},
    {"data_in=x model_write=device model_out=m shards=2 exchange=split", 0, "", 1, 0},
    {"data_in=x model_write=device task=2 model_in=m data_val=v", 0, "", 1, 0},
    {"data_in=x model_write=Device", 2, VALUE, kAny, kAny},
    {"data_in=x model_write=", 2, VALUE, kAny, kAny},
    {"data_in=x model_write=gpu model_out=m", 2, VALUE, kAny, kAny},
    {"data_in=x model_write=1 shards=2", 2, VALUE, kAny, kAny},
    // ---- task=1: data_in is not needed, model_in is, shards are refused
    {"task=1 model_in=m", 0, "", 0, 1},
    {"task=1 model_in=m V_dim=4", 0, "", 0, 1},
    {"task=1 model_in=m model_write=device", 0, "", 1, 1},
    {"task=1 model_in=m model_write=device name_dump=d.txt need_reverse=1 dump_aux=1", 0, "", 1, 1},
    {"task=1 model_in=m data_in=x", 0, "", 0, 1},
    {"task=1 model_in=m fused=0", 0, "", 0, 1},
    {"task=1", 2, NEEDS_IN, kAny, kAny},
    {"task=1 data_in=x", 2, NEEDS_IN, kAny, kAny},
    {"task=1 model_out=m", 2, NEEDS_IN, kAny, kAny},
    {"task=1 model_in=m shards=2", 2, NEEDS_SINGLE, kAny, kAny},
    {"task=1 model_in=m shards=-1", 2, NEEDS_SINGLE, kAny, kAny},
    {"task=1 model_in=m shards=2 exchange=split", 2, NEEDS_SINGLE, kAny, kAny},
    {"task=1 shards=2", 2, NEEDS_IN, kAny, kAny},
    // ---- the value rule before task=1's, and both behind every older refusal
    {"task=1 model_write=bogus", 2, VALUE, kAny, kAny},
    {"task=1 model_in=m shards=2 model_write=bogus", 2, VALUE, kAny, kAny},
    {"task=1 parse=bogus", 2, "parse must be host, device, auto or auto-sharded", kAny, kAny},
    {"task=1 model_write=bogus cache=bogus", 2, "cache must be none, device or auto", kAny, kAny},
    {"task=1 model_write=bogus pred_write=bogus", 2, "pred_write must be host or device", kAny,
     kAny},
    {"task=1 model_in=m shards=2 exchange=bogus", 2, "exchange must be a2a or split", kAny, kAny},
    {"data_in=x model_write=bogus shards=2 exchange=bogus", 2, "exchange must be a2a or split",
     kAny, kAny},
    {"data_in=x model_write=bogus task=2", 2, "prediction needs model_in and data_val", kAny, kAny},
    {"data_in=x model_write=bogus pred_write=device fused=0", 2,
     "pred_write=device needs the fused path (fused=1): the interface path keeps its predictions "
     "on the host",
     kAny, kAny},
    {"data_in=x model_write=bogus parse=device", 2,
     "parse=device needs data_format=criteo or criteo_test", kAny, kAny},
};
}  // namespace

int main() {
  for (const Row& row : kRows) {
    const Resolved r = Resolve(row.args);
    const bool ok = r.rc == row.rc && r.err == row.err &&
                    (row.device == kAny || ((int)r.plan.model_write_device == row.device &&
                                            (int)r.plan.dump == row.dump));
    if (!ok) {
      ++failures;
      std::printf("FAILED [%s]: rc %d err '%s' device %d dump %d, expected %d '%s' %d %d\n",
                  row.args, r.rc, r.err.c_str(), (int)r.plan.model_write_device, (int)r.plan.dump,
                  row.rc, row.err, row.device, row.dump);
    }
    if (!r.parsed) {
      ++failures;
      std::printf("FAILED [%s]: ParseArgs refused it: '%s'\n", row.args, r.err.c_str());
    }
    // the new keys are Param's: only fused and V_dim go on to the context
    const std::string a(row.args);
    const size_t other = (a.find("fused=") != std::string::npos) +
                         (a.find("V_dim=") != std::string::npos);
    if (r.rest != other) {
      ++failures;
      std::printf("FAILED [%s]: %zu keys Param did not know\n", row.args, r.rest);
    }
  }
  // no data_in: still the usage error for every task but 1 and 2
  for (const char* args : {"", "task=0", "task=3 model_in=m", "model_write=device"}) {
    const Resolved r = Resolve(args);
    if (r.parsed || r.rc != 2 || r.err.find("usage:") != 0) {
      ++failures;
      std::printf("FAILED [%s]: expected the usage error, got rc %d '%s'\n", args, r.rc,
                  r.err.c_str());
    }
  }
  {
    const Resolved r =
        Resolve("task=1 model_in=m name_dump=out.txt need_reverse=1 dump_aux=1 model_write=device");
    if (r.P.name_dump != "out.txt" || !r.P.need_reverse || !r.P.dump_aux || r.P.task != 1) {
      ++failures;
      std::printf("FAILED: task=1's keys did not reach Param\n");
    }
  }
  const Param dflt;
  if (dflt.model_write != "host" || dflt.name_dump != "dump.txt" || dflt.need_reverse ||
      dflt.dump_aux) {
    ++failures;
    std::printf("FAILED: the defaults are not model_write=host name_dump=dump.txt need_reverse=0 "
                "dump_aux=0\n");
  }
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("train_options_model_tests: ALL PASSED (%zu rows)\n",
              sizeof(kRows) / sizeof(kRows[0]));
  return 0;
}
