# Builds libwindtunnel.so and libwtpolar.so (HIP, gfx950) in-tree and the C oracle (test infrastructure).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
PKG       = airfoil-cfd-tool_amd
CSRC      = $(PKG)/csrc
LIB       = $(PKG)/lib/libwindtunnel.so
POLAR     = $(PKG)/lib/libwtpolar.so
# -ffp-contract=off: one rounding per operation, as the oracle (and the parity tests) assume.
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wno-unused-function
# EXPERIMENT=1: the planner / launch-order environment knobs of tools/ (include/windtunnel.h "Environment"); never for a production build
ifeq ($(EXPERIMENT),1)
HIPFLAGS += -DWT_EXPERIMENT_KNOBS
endif
# No -lrccl: the RCCL entry points are bound at the first wt_comm_* call to the ONE RCCL the process has mapped (csrc/rccl_bind.hpp); the run path is
# for processes without PyTorch, where that call has to dlopen librccl.so.1 itself.
LDFLAGS  ?= -ldl -Wl,-rpath,/opt/rocm/lib -Wl,--version-script=$(CSRC)/libwindtunnel.map
POLAR_LDFLAGS ?= -Wl,-rpath,/opt/rocm/lib -Wl,--version-script=$(CSRC)/libwtpolar.map

all: lib oracle

lib: $(LIB) $(POLAR)

# (the batch source is not a prerequisite of libwindtunnel.so: editing it does not rebuild the single-tunnel library)
$(LIB): $(filter-out $(CSRC)/polar.hip,$(wildcard $(CSRC)/*.hip)) $(wildcard $(CSRC)/*.hpp) $(CSRC)/libwindtunnel.map include/windtunnel.h
	mkdir -p $(PKG)/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(CSRC)/windtunnel.hip $(LDFLAGS)

# batched sweeps (include/wt_polar.h): a library of its own, so that libwindtunnel.so's export list stays that of windtunnel.h
$(POLAR): $(CSRC)/polar.hip $(wildcard $(CSRC)/*.hpp) $(CSRC)/libwtpolar.map include/wt_polar.h include/windtunnel.h
	mkdir -p $(PKG)/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(CSRC)/polar.hip $(POLAR_LDFLAGS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(PKG)/lib oracle/_build
.PHONY: all lib oracle clean
