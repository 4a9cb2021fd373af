# Builds libdifacto_amd.so (gfx950 HIP kernels + the C-ABI), the oracle (test
# infrastructure), and the C++ host adapters/tests.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# -ffp-contract=off: the reference computes without FMA contraction; parity needs the same
HIPFLAGS = --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -ffp-contract=off -Wall -Wno-unused-function
CSRC = difacto_amd/csrc
OBJDIR = build/obj
SRCS = $(wildcard $(CSRC)/*.hip)
OBJS = $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
HDRS = $(wildcard $(CSRC)/*.h) include/difacto_amd.h
LIB = difacto_amd/libdifacto_amd.so

HOSTBIN = build/host_tests
TRAINBIN = build/dfx_train
HOSTLIB = difacto_amd/host/gpu_adapters.cc difacto_amd/host/reader.cc \
  difacto_amd/host/device_reader.cc
# CityHash64, one text for reader.cc and the device parser (textparse.hip)
CITYHDR = $(CSRC)/cityhash.h
HOSTSRC = $(HOSTLIB) difacto_amd/host/dist_store.cc difacto_amd/host/split_learner.cc \
  tests/host/host_tests.cc
HOSTHDR = difacto_amd/host/iface.h difacto_amd/host/gpu_adapters.h difacto_amd/host/reader.h \
  difacto_amd/host/dist_host.h difacto_amd/host/dist_store.h difacto_amd/host/split_learner.h \
  difacto_amd/host/device_reader.h difacto_amd/host/train_options.h include/difacto_amd.h \
  include/difacto_amd_dist.h $(CITYHDR) $(CSRC)/reshuffle.h
HOSTFLAGS = -std=c++14 -O2 -Wall -pthread

READERBIN = build/reader_tests
GENBIN = build/gen_criteo
CONVBIN = build/dfx_convert
RBENCH = build/reader_bench
TPBIN = build/textparse_tests
LSBIN = build/libsvmparse_tests
ADBIN = build/adfeaparse_tests
SEBIN = build/shard_eval_tests
SDBIN = build/split_device_tests
SPBIN = build/shard_parse_tests

DISTLIB = difacto_amd/libdfx_dist.so

all: $(LIB) $(DISTLIB) oracle $(HOSTBIN) $(TRAINBIN) $(READERBIN) $(GENBIN) $(CONVBIN) $(RBENCH) \
  $(TPBIN) $(LSBIN) $(ADBIN) $(SEBIN) $(SDBIN) $(SPBIN) build/expf_check build/strtof_check \
  build/gen_libsvm build/locbench \
  build/reshuffle_check build/resample_check build/fmtg_check build/train_options_tests \
  build/train_options_resample_tests build/train_options_adfea_tests build/gen_adfea \
  build/modeltext_check build/train_options_model_tests

$(RBENCH): difacto_amd/host/reader.cc tools/reader_bench.cc difacto_amd/host/reader.h $(CITYHDR)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ difacto_amd/host/reader.cc tools/reader_bench.cc

# the data converter (src/reader/converter.h): text formats -> rec (CompressedRowBlock RecordIO)
$(CONVBIN): difacto_amd/host/reader.cc difacto_amd/host/convert_main.cc difacto_amd/host/reader.h \
  difacto_amd/host/iface.h $(CITYHDR)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ difacto_amd/host/reader.cc difacto_amd/host/convert_main.cc

$(GENBIN): tools/gen_criteo.cc
	@mkdir -p build
	g++ -O2 -o $@ $<

# the readers alone (CPU only: no libdifacto_amd)
$(READERBIN): difacto_amd/host/reader.cc tests/host/reader_tests.cc difacto_amd/host/reader.h \
  difacto_amd/host/iface.h $(CITYHDR)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ difacto_amd/host/reader.cc tests/host/reader_tests.cc -ldl

# dfx_train's option rules alone (CPU only, no library): ResolveOptions' truth table
build/train_options_tests: tests/host/train_options_tests.cc difacto_amd/host/train_options.h \
  difacto_amd/host/iface.h
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ tests/host/train_options_tests.cc

# ... and epoch_resample's rules, behind epoch_shuffle's
build/train_options_resample_tests: tests/host/train_options_resample_tests.cc \
  difacto_amd/host/train_options.h difacto_amd/host/iface.h
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ tests/host/train_options_resample_tests.cc

# ... and parse_adfea's, beside the parse value's
build/train_options_adfea_tests: tests/host/train_options_adfea_tests.cc \
  difacto_amd/host/train_options.h difacto_amd/host/iface.h
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ tests/host/train_options_adfea_tests.cc

# ... and model_write's and task=1's, behind every older rule
build/train_options_model_tests: tests/host/train_options_model_tests.cc \
  difacto_amd/host/train_options.h difacto_amd/host/iface.h
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ tests/host/train_options_model_tests.cc

# the device text parser, the row gather and DeviceBatchReader against the host reader
# (dfx_parse_criteo / dfx_gather_rows vs ParseCriteo / GatherRows / BatchReader), plus the CPU
# modes: the batch planner, the raw-mode chunk cuts, the shared CityHash64
$(TPBIN): $(HOSTLIB) tests/host/textparse_tests.cc $(HOSTHDR) $(LIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) tests/host/textparse_tests.cc -Ldifacto_amd -ldifacto_amd \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# the device libsvm parser, the valued row gather and DeviceBatchReader("libsvm") against the
# host reader (dfx_parse_libsvm / dfx_gather_rows_valued vs ParseLibSVM / GatherRows /
# BatchReader), plus the CPU mode: the batch planner on valued rows with the flag mirroring
$(LSBIN): $(HOSTLIB) tests/host/libsvmparse_tests.cc $(HOSTHDR) $(CSRC)/strtof.h $(LIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) tests/host/libsvmparse_tests.cc -Ldifacto_amd -ldifacto_amd \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# the device adfea parser, the adfea text feed and DeviceBatchReader("adfea") against the host
# reader (dfx_parse_adfea vs ParseAdfea / BatchReader), plus the CPU mode: the batch planner on
# binary rows of varying length
$(ADBIN): $(HOSTLIB) tests/host/adfeaparse_tests.cc $(HOSTHDR) $(LIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) tests/host/adfeaparse_tests.cc -Ldifacto_amd -ldifacto_amd \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# test infrastructure: csrc/strtof.h (the device parser's numbers) against the host's strtof
build/strtof_check: tools/strtof_check.cc $(CSRC)/strtof.h
	@mkdir -p build
	g++ -std=c++14 -O2 -Wall -o $@ $<

# test infrastructure: csrc/reshuffle.h (the reshuffler's permutation) printed from the host
build/reshuffle_check: tools/reshuffle_check.cc $(CSRC)/reshuffle.h
	@mkdir -p build
	g++ -std=c++14 -O2 -Wall -o $@ $<

# test infrastructure: csrc/reshuffle.h's per-epoch down-sample (rs_draw, rs_dropped) from the host
build/resample_check: tools/resample_check.cc $(CSRC)/reshuffle.h
	@mkdir -p build
	g++ -std=c++14 -O2 -Wall -o $@ $<

# test infrastructure: csrc/fmtg.h (the device prediction writer's rows) against the host's
# snprintf("%g") and the driver's probability expression; also writes the GPU tests' expected text
build/fmtg_check: tools/fmtg_check.cc $(CSRC)/fmtg.h $(CSRC)/expf.h
	@mkdir -p build
	g++ -std=c++17 -O2 -Wall -ffp-contract=off -o $@ $<

# test infrastructure: csrc/modeltext.h (the device model dump's lines) against a std::ostream
build/modeltext_check: tools/modeltext_check.cc $(CSRC)/modeltext.h $(CSRC)/fmtg.h \
  $(CSRC)/revbytes.h $(CSRC)/expf.h
	@mkdir -p build
	g++ -std=c++17 -O2 -Wall -ffp-contract=off -o $@ $<

build/gen_libsvm: tools/gen_libsvm.cc
	@mkdir -p build
	g++ -O2 -o $@ $<

build/gen_adfea: tools/gen_adfea.cc
	@mkdir -p build
	g++ -O2 -o $@ $<

# C++ host adapters (the reference's Loss/Updater/Store over the C-ABI) + their test driver;
# plain g++ against the C-ABI (the sharded store's exchange, dist_host.o, links RCCL)
$(HOSTBIN): $(HOSTSRC) $(HOSTHDR) build/obj/dist_host.o $(LIB) $(DISTLIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTSRC) build/obj/dist_host.o -Ldifacto_amd -ldifacto_amd -ldfx_dist \
	  -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# the sharded stores' evaluation paths from C++ (GpuShardedStore's non-training branch,
# GpuSplitLearner's prediction output) against the single context's validation step
$(SEBIN): $(HOSTLIB) difacto_amd/host/split_learner.cc tests/host/shard_eval_tests.cc $(HOSTHDR) \
  build/obj/dist_host.o $(LIB) $(DISTLIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) difacto_amd/host/split_learner.cc \
	  tests/host/shard_eval_tests.cc build/obj/dist_host.o \
	  -Ldifacto_amd -ldifacto_amd -ldfx_dist -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# GpuSplitLearner's device entry (ProcessDeviceBatches: device, mixed and replayed steps) against
# the same steps fed host row blocks, bit for bit
$(SDBIN): $(HOSTLIB) difacto_amd/host/split_learner.cc tests/host/split_device_tests.cc $(HOSTHDR) \
  build/obj/dist_host.o $(LIB) $(DISTLIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $(HOSTLIB) \
	  difacto_amd/host/split_learner.cc tests/host/split_device_tests.cc build/obj/dist_host.o \
	  -Ldifacto_amd -ldifacto_amd -ldfx_dist -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# both sharded stores fed by DeviceBatchReaders (late marking of the text feed's ring entries and
# slots) against the same stores fed the host reader's blocks, bit for bit
$(SPBIN): $(HOSTLIB) difacto_amd/host/split_learner.cc tests/host/shard_parse_tests.cc $(HOSTHDR) \
  build/obj/dist_host.o $(LIB) $(DISTLIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) difacto_amd/host/split_learner.cc \
	  tests/host/shard_parse_tests.cc build/obj/dist_host.o \
	  -Ldifacto_amd -ldifacto_amd -ldfx_dist -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# the sharded store's C++ driver (host code: HIP runtime API + RCCL, built by hipcc)
build/obj/dist_host.o: difacto_amd/host/dist_host.cc difacto_amd/host/dist_host.h include/difacto_amd.h
	@mkdir -p build/obj
	$(HIPCC) -std=c++17 -O2 -fPIC -Wall -c $< -o $@

# the training driver (src/main.cc + SGDLearner::RunScheduler): reader -> feeder -> fused step,
# or the sharded store over RCCL / loopback
$(TRAINBIN): $(HOSTLIB) difacto_amd/host/train_main.cc difacto_amd/host/split_learner.cc \
  $(HOSTHDR) difacto_amd/host/dist_host.h build/obj/dist_host.o $(LIB) $(DISTLIB)
	@mkdir -p build
	g++ $(HOSTFLAGS) -o $@ $(HOSTLIB) difacto_amd/host/train_main.cc \
	  difacto_amd/host/split_learner.cc build/obj/dist_host.o \
	  -Ldifacto_amd -ldifacto_amd -ldfx_dist -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN/../difacto_amd' -Wl,-rpath,/opt/rocm/lib

# the multi-GPU split driver's C-ABI (include/difacto_amd_dist.h): host code (HIP runtime
# API + RCCL) over libdifacto_amd.so, loaded by difacto_amd/_lib.py beside it
$(DISTLIB): difacto_amd/host/split_host.cc difacto_amd/host/split_host.h \
  include/difacto_amd_dist.h include/difacto_amd.h $(LIB)
	g++ -std=c++17 -O2 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -shared -o $@ \
	  difacto_amd/host/split_host.cc -Ldifacto_amd -ldifacto_amd -L/opt/rocm/lib -lrccl -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -s -C oracle

# measurement: the fused step's Localizer alone (links the library's internals)
build/locbench: tools/locbench.hip $(LIB) $(HDRS)
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wno-unused-result -o $@ $< -Ldifacto_amd \
	  -ldifacto_amd -Wl,-rpath,'$$ORIGIN/../difacto_amd'

# test infrastructure: the device's expf (csrc/expf.h) against the host's glibc expf
build/expf_check: tools/expf_check.hip $(CSRC)/expf.h
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -ffp-contract=off -o $@ $<

# measurement: the model files' host writers against the device writers, A B B A (needs a GPU)
model_write_ab: $(LIB)
	python tools/model_write_ab.py

clean:
	rm -rf build $(LIB) $(DISTLIB)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean model_write_ab
