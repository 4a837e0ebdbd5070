# Build of the MI355X stem-kernel engine (gfx950) and the test oracle.
#   make            -> stem_kernel_amd/libstem_kernel_amd.so + oracle
#   make lib        -> product library only
#   make oracle     -> oracle/liboracle.so (+ oracle/_ref when /root/reference exists)
ROOT := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
JOBS ?= 8
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -I$(ROOT)include -I$(ROOT)stem_kernel_amd/csrc
HIPFLAGS := $(CXXFLAGS) --offload-arch=$(ARCH) -munsafe-fp-atomics
BUILD := $(ROOT)build
LIB := $(ROOT)stem_kernel_amd/libstem_kernel_amd.so
LINK := $(HIPCC) --offload-arch=$(ARCH) -shared -fPIC
LINK_LIBS := -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

HOST_SRC := $(ROOT)stem_kernel_amd/csrc/host/synth.cpp $(ROOT)stem_kernel_amd/csrc/host/example_build.cpp \
            $(ROOT)stem_kernel_amd/csrc/host/readers.cpp $(ROOT)stem_kernel_amd/csrc/host/shard.cpp \
            $(ROOT)stem_kernel_amd/csrc/host/svm_predict.cpp $(ROOT)stem_kernel_amd/csrc/host/fold_host.cpp \
            $(ROOT)stem_kernel_amd/csrc/host/svm_train.cpp $(ROOT)stem_kernel_amd/csrc/host/auc_gradient.cpp \
            $(ROOT)stem_kernel_amd/csrc/host/feature_gram.cpp
# the host runtime behind the ABI (they share host/runtime.h, host/runtime_types.h)
API_SRC := $(ROOT)stem_kernel_amd/csrc/sk_api.cpp $(addprefix $(ROOT)stem_kernel_amd/csrc/host/,context.cpp pack.cpp pack_x.cpp pack_y.cpp pack_sweep.cpp pack_shared_sums.cpp \
           dataset.cpp dataset_io.cpp fold_gpu.cpp pairs_dag.cpp pairs_bpla.cpp pairs_la_protein.cpp \
           pairs_simpal.cpp pairs_stem4d.cpp la_protein_grad.cpp stem_grad.cpp pairs_stem_grad.cpp)
HIP_SRC := $(ROOT)stem_kernel_amd/csrc/kernels/dag_stem.hip $(ROOT)stem_kernel_amd/csrc/kernels/profile_string.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/bpla.hip $(ROOT)stem_kernel_amd/csrc/kernels/stem4d.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/phmm.hip $(ROOT)stem_kernel_amd/csrc/kernels/bpla_grad.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/dag_stem_big.hip $(ROOT)stem_kernel_amd/csrc/kernels/fold.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/fold_sample.hip $(ROOT)stem_kernel_amd/csrc/kernels/fold_ali.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/la_protein.hip $(ROOT)stem_kernel_amd/csrc/kernels/simpal.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/svm_smo.hip $(ROOT)stem_kernel_amd/csrc/kernels/auc_grad.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/feature_gram.hip $(ROOT)stem_kernel_amd/csrc/kernels/la_protein_grad.hip \
           $(ROOT)stem_kernel_amd/csrc/kernels/stem_grad.hip
HDRS := $(wildcard $(ROOT)stem_kernel_amd/csrc/*/*.h) $(ROOT)include/stem_kernel.h $(ROOT)stem_kernel_amd/csrc/ribosum85_60.inc \
        $(ROOT)stem_kernel_amd/csrc/blosum62.inc

HOST_OBJ := $(patsubst $(ROOT)stem_kernel_amd/csrc/%.cpp,$(BUILD)/%.o,$(HOST_SRC) $(API_SRC))
HIP_OBJ := $(patsubst $(ROOT)stem_kernel_amd/csrc/%.hip,$(BUILD)/%.o,$(HIP_SRC))

all: lib cli oracle exp

lib: $(LIB)

# the reference's stem_kernel_lite CLI over the engine (host C++, links the library)
CLI := $(ROOT)stem_kernel_amd/bin/stem_kernel_lite
cli: $(CLI)
$(CLI): $(ROOT)stem_kernel_amd/csrc/cli/stem_kernel_lite.cpp $(ROOT)include/stem_kernel_compat.hpp $(ROOT)include/stem_kernel.h $(LIB)
	@mkdir -p $(dir $@)
	g++ -O2 -std=c++17 -Wall -Wextra -I$(ROOT)include $< -L$(ROOT)stem_kernel_amd -lstem_kernel_amd -lz -ldl \
	  -Wl,-rpath,'$$ORIGIN/..' -o $@

$(BUILD)/%.o: $(ROOT)stem_kernel_amd/csrc/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -c $< -o $@

$(BUILD)/%.o: $(ROOT)stem_kernel_amd/csrc/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

# the PairHMM's log-space sums must round like the host restatement
$(BUILD)/kernels/phmm.o: HIPFLAGS += -ffp-contract=off
$(BUILD)/kernels/bpla_grad.o: HIPFLAGS += -ffp-contract=off
# the synthetic fold's AVX2 clone and baseline must round alike (no FMA)
$(BUILD)/host/synth.o: CXXFLAGS += -ffp-contract=off
# the SMO solver's G update has four roundings, on the host and in the kernel
$(BUILD)/host/svm_train.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/kernels/svm_smo.o: HIPFLAGS += -ffp-contract=off
# the AUC gradient's conjugate gradient amplifies rounding: both paths round every operation alone
$(BUILD)/host/auc_gradient.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/kernels/auc_grad.o: HIPFLAGS += -ffp-contract=off
# the feature-vector dot is libsvm's sparse merge bit for bit: multiply, then add, on both paths
$(BUILD)/host/feature_gram.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/kernels/feature_gram.o: HIPFLAGS += -ffp-contract=off
# the protein LA gradients' host path restates the reference operation by operation
$(BUILD)/host/la_protein_grad.o: CXXFLAGS += -ffp-contract=off
# the stem gradients' host path restates the reference's DP operation by operation
$(BUILD)/host/stem_grad.o: CXXFLAGS += -ffp-contract=off

$(LIB): $(HOST_OBJ) $(HIP_OBJ)
	$(LINK) -o $@ $^ $(LINK_LIBS)

oracle:
	$(MAKE) -C $(ROOT)oracle

clean:
	rm -rf $(BUILD) $(LIB) $(CLI)
	$(MAKE) -C $(ROOT)oracle clean

.PHONY: all lib cli oracle clean

# The diagnostic and experiment builds below recompile some sources with
# extra defines and link them with the default build's other objects (make lib
# first): $(call relink,out.so,replaced default objects,their replacements)
relink = $(LINK) -o $(1) $(filter-out $(2),$(HOST_OBJ) $(HIP_OBJ)) $(3) $(LINK_LIBS)
# the default objects of the host runtime (API_SRC), and the same set under a build directory
API_OBJ := $(patsubst $(ROOT)stem_kernel_amd/csrc/%.cpp,$(BUILD)/%.o,$(API_SRC))
api_obj = $(patsubst $(BUILD)/%.o,$(1)/%.o,$(API_OBJ))

# diagnostic build with in-kernel phase stamps (never the shipped library)
STAMPS_LIB := $(ROOT)build/libstem_kernel_amd_stamps.so
$(BUILD)/stamps/%.o: $(ROOT)stem_kernel_amd/csrc/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -DSK_STAMPS -D__HIP_PLATFORM_AMD__ -c $< -o $@
stamps: $(call api_obj,$(BUILD)/stamps)
	$(HIPCC) $(HIPFLAGS) -DSK_STAMPS -x hip -c $(ROOT)stem_kernel_amd/csrc/kernels/dag_stem.hip -o $(BUILD)/stamps/dag_stem.o
	$(call relink,$(STAMPS_LIB),$(API_OBJ) $(BUILD)/kernels/dag_stem.o,$(call api_obj,$(BUILD)/stamps) $(BUILD)/stamps/dag_stem.o)
.PHONY: stamps

# experiment build: make variant NAME=x DEFS="-DSK_PW=3 [-DSK_STAMPS]" -> build/libsk_x.so
# (the objects of a NAME are rebuilt on every call, FORCE: another DEFS may go
# by the same NAME, where the stamps objects have one set of defines and
# follow their sources like the default build's)
ifneq ($(NAME),)
$(BUILD)/var/$(NAME)/%.o: $(ROOT)stem_kernel_amd/csrc/%.cpp $(HDRS) FORCE
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) $(DEFS) -D__HIP_PLATFORM_AMD__ -c $< -o $@
endif
variant: $(call api_obj,$(BUILD)/var/$(NAME))
	$(HIPCC) $(HIPFLAGS) $(DEFS) -x hip -c $(ROOT)stem_kernel_amd/csrc/kernels/dag_stem.hip -o $(BUILD)/var/$(NAME)/dag_stem.o
	$(call relink,$(BUILD)/libsk_$(NAME).so,$(API_OBJ) $(BUILD)/kernels/dag_stem.o,$(call api_obj,$(BUILD)/var/$(NAME)) $(BUILD)/var/$(NAME)/dag_stem.o)
FORCE:
.PHONY: variant FORCE

# fold kernel experiment build: make variantf NAME=x DEFS="-DSK_FOLD_TIMING" -> build/libsk_x.so
variantf:
	@mkdir -p $(BUILD)/var/$(NAME)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -x hip -c $(ROOT)stem_kernel_amd/csrc/kernels/fold.hip -o $(BUILD)/var/$(NAME)/fold.o
	$(call relink,$(BUILD)/libsk_$(NAME).so,$(BUILD)/kernels/fold.o,$(BUILD)/var/$(NAME)/fold.o)
.PHONY: variantf

# 4-D kernel experiment build: make variant4 NAME=x DEFS="-DSK4_MINB=4" -> build/libsk_x.so
variant4:
	@mkdir -p $(BUILD)/var/$(NAME)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -x hip -c $(ROOT)stem_kernel_amd/csrc/kernels/stem4d.hip -o $(BUILD)/var/$(NAME)/stem4d.o
	$(call relink,$(BUILD)/libsk_$(NAME).so,$(BUILD)/kernels/stem4d.o,$(BUILD)/var/$(NAME)/stem4d.o)
.PHONY: variant4

# experiments build: the shipped sources with the A/B switches compiled in
# (SK_KNOB reads the environment; sk_experiments() = 1) -> build/libstem_kernel_amd_exp.so,
# loaded by the GPU tests that compare kernel variants (tests/explib.py)
EXP_LIB := $(ROOT)build/libstem_kernel_amd_exp.so
EXP_OBJ := $(patsubst $(ROOT)stem_kernel_amd/csrc/%.cpp,$(BUILD)/exp/%.o,$(HOST_SRC) $(API_SRC))
exp: $(EXP_LIB)
$(BUILD)/exp/%.o: $(ROOT)stem_kernel_amd/csrc/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(CXXFLAGS) -DSK_EXPERIMENTS -D__HIP_PLATFORM_AMD__ -c $< -o $@
$(BUILD)/exp/host/synth.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/exp/host/svm_train.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/exp/host/auc_gradient.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/exp/host/feature_gram.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/exp/host/la_protein_grad.o: CXXFLAGS += -ffp-contract=off
$(BUILD)/exp/host/stem_grad.o: CXXFLAGS += -ffp-contract=off
$(EXP_LIB): $(EXP_OBJ) $(HIP_OBJ)
	$(LINK) -o $@ $^ $(LINK_LIBS)
.PHONY: exp
