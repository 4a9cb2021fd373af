// train_options_adfea_tests.cc — parse_adfea's rows of dfx_train's option rules (CPU only, no
// library; train_options_tests.cc holds the table of every other option): the key across
// parse=host|device|auto|auto-sharded, shards=0|2, fused=0|1 and data_format=adfea|libsvm|criteo
// against the exit status, the stderr message, the stdout lines and the plan's parse.  With
// parse_adfea=0 the adfea rows are the ones the older tests pin; with 1 adfea is a format with a
// device parser and every rule of auto / auto-sharded applies to it unchanged; the two refusals
// stand right behind the parse value's and before everything else.
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
  std::string err, lines;  // the lines joined, each with its '\n'
  RunPlan plan;
  size_t rest;  // keys Param did not know (fused is one)
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
  for (const auto& l : lines) r.lines += l + "\n";
  return r;
}

const int kAny = -1, kHost = 0, kDev = 1;

struct Row {
  const char* args;
  int rc;
  const char* err;    // the whole message
  const char* lines;  // the whole stdout
  int parse;          // the plan's (kAny: a refused row)
};

#define NEEDS_FORMAT "parse_adfea=1 needs data_format=adfea"
#define NEEDS_AUTO "parse_adfea=1 needs parse=auto or parse=auto-sharded"
#define HOST_ADFEA "parse: host (data_format=adfea)\n"

const Row kRows[] = {
    // ---- parse_adfea=0 (and the key absent): the adfea lines as they were
    {"data_format=adfea", 0, "", "", kHost},
    {"data_format=adfea parse=host", 0, "", "", kHost},
    {"data_format=adfea parse=auto", 0, "", HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto parse_adfea=0", 0, "", HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto-sharded parse_adfea=0", 0, "", HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto-sharded shards=2", 0, "", HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto-sharded shards=2 parse_adfea=0", 0, "", HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto-sharded shards=2 exchange=split parse_adfea=0", 0, "",
     HOST_ADFEA, kHost},
    {"data_format=adfea parse=auto shards=2 parse_adfea=0", 0, "", "parse: host (a sharded run)\n",
     kHost},
    {"data_format=adfea parse=auto fused=0 parse_adfea=0", 0, "", "parse: host (fused=0)\n", kHost},
    {"data_format=adfea parse=device parse_adfea=0", 2,
     "parse=device needs data_format=criteo or criteo_test", "", kAny},
    {"data_format=adfea parse=host parse_adfea=0 shards=2", 0, "", "", kHost},
    {"data_format=libsvm parse=auto parse_adfea=0", 0, "", "parse: device (libsvm)\n", kDev},
    {"data_format=criteo parse=device parse_adfea=0", 0, "", "", kDev},
    // ---- parse_adfea=1, data_format=adfea, parse=auto: every rule of auto
    {"data_format=adfea parse=auto parse_adfea=1", 0, "", "parse: device (adfea)\n", kDev},
    {"data_format=adfea parse=auto parse_adfea=1 fused=1", 0, "", "parse: device (adfea)\n", kDev},
    {"data_format=adfea parse=auto parse_adfea=1 fused=0", 0, "", "parse: host (fused=0)\n", kHost},
    {"data_format=adfea parse=auto parse_adfea=1 shards=2", 0, "", "parse: host (a sharded run)\n",
     kHost},
    {"data_format=adfea parse=auto parse_adfea=1 shards=2 fused=0", 0, "",
     "parse: host (a sharded run)\n", kHost},
    {"data_format=adfea parse=auto parse_adfea=1 shards=2 exchange=split", 0, "",
     "parse: host (exchange=split)\n", kHost},
    // ---- ... parse=auto-sharded: auto without shards, the device parser per shard with
    {"data_format=adfea parse=auto-sharded parse_adfea=1", 0, "", "parse: device (adfea)\n", kDev},
    {"data_format=adfea parse=auto-sharded parse_adfea=1 fused=0", 0, "",
     "parse: host (fused=0)\n", kHost},
    {"data_format=adfea parse=auto-sharded parse_adfea=1 shards=2", 0, "",
     "parse: device (adfea, 2 shards)\n", kDev},
    {"data_format=adfea parse=auto-sharded parse_adfea=1 shards=2 exchange=split", 0, "",
     "parse: device (adfea, 2 shards)\n", kDev},
    {"data_format=adfea parse=auto-sharded parse_adfea=1 shards=2 fused=0", 0, "",
     "parse: device (adfea, 2 shards)\n", kDev},
    // ---- the refusals: the format first, then the parse value; behind "parse must be"
    {"parse_adfea=1 parse=bogus", 2, "parse must be host, device, auto or auto-sharded", "", kAny},
    {"parse_adfea=1 parse=bogus data_format=adfea", 2,
     "parse must be host, device, auto or auto-sharded", "", kAny},
    {"parse_adfea=1", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=auto", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=auto data_format=libsvm", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=auto-sharded shards=2 data_format=libsvm", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=auto data_format=criteo", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=device data_format=criteo", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 parse=host data_format=criteo fused=0 shards=2", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 data_format=adfea", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=host", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=host shards=2", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=host fused=0", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=device", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=device shards=2 fused=0", 2, NEEDS_AUTO, "", kAny},
    // ---- ... and before every later rule; a later refusal leaves the parse line out
    {"parse_adfea=1 cache=bogus", 2, NEEDS_FORMAT, "", kAny},
    {"parse_adfea=1 data_format=adfea cache_loc=1", 2, NEEDS_AUTO, "", kAny},
    {"parse_adfea=1 data_format=adfea parse=auto cache=bogus", 2,
     "cache must be none, device or auto", "parse: device (adfea)\n", kAny},
    // ---- with the cache
    {"parse_adfea=1 data_format=adfea parse=auto cache=device", 0, "", "parse: device (adfea)\n",
     kDev},
    {"parse_adfea=1 data_format=adfea parse=auto-sharded shards=2 cache=auto", 0, "",
     "parse: device (adfea, 2 shards)\ncache: device (exchange=a2a)\n", kDev},
};
}  // namespace

int main() {
  for (const Row& row : kRows) {
    const Resolved r = Resolve(row.args);
    const bool ok = r.rc == row.rc && r.err == row.err && r.lines == row.lines &&
                    (row.parse == kAny ||
                     (int)(r.plan.parse == RunPlan::Parse::kDevice) == row.parse);
    if (!ok) {
      ++failures;
      std::printf("FAILED [%s]: rc %d err '%s' lines '%s' parse %d, expected %d '%s' '%s' %d\n",
                  row.args, r.rc, r.err.c_str(), r.lines.c_str(),
                  (int)(r.plan.parse == RunPlan::Parse::kDevice), row.rc, row.err, row.lines,
                  row.parse);
    }
    // parse_adfea is a key of Param's: only fused goes on to the context
    const size_t fused_keys = std::string(row.args).find("fused=") != std::string::npos;
    if (r.rest != fused_keys) {
      ++failures;
      std::printf("FAILED [%s]: %zu keys Param did not know\n", row.args, r.rest);
    }
  }
  if (Param().parse_adfea) {
    ++failures;
    std::printf("FAILED: parse_adfea is not off by default\n");
  }
  if (failures) {
    std::printf("%d FAILED\n", failures);
    return 1;
  }
  std::printf("train_options_adfea_tests: ALL PASSED (%zu rows)\n",
              sizeof(kRows) / sizeof(kRows[0]));
  return 0;
}
