# pgo_check: the host side of loop closure (tests/c/pgo_check.cpp): rspl_pgo_debug_host, rspl_pgo_debug_plan, the
# refusals, the three map calls, and the layout of the four rspl_pgo_* structs.  It makes no device call, so it runs
# without a GPU.
#   make -C tests/c -f pgo_check.mk pgo_check       build/pgo_check: pgo_check.cpp linked with the built librspl.so;
#                                                   tests/test_pgo_cpu.py builds and runs it
#   make -C tests/c -f pgo_check.mk pgo_check_san   build/pgo_check_san, on demand.  Under ASan + UBSan (host code):
#                                                   pgo_check.cpp, pgo.cpp, pgo_kernels.hip, map.cpp, common.cpp --
#                                                   every function pgo_check calls is defined in these, and its calls
#                                                   bind to these definitions at link time.  map.cpp also refers to
#                                                   the BA and keyframe handles (rspl_map_local_optimization,
#                                                   rspl_map_insert_keyframe), which pgo_check never calls; only
#                                                   those references are met by librspl.so, unsanitised.  (reloc_check
#                                                   links objects alone because lmap_reloc.cpp has no such references.)
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
PKG := $(ROOT)/rspl-slam_amd
CSRC := $(PKG)/csrc
ROCM ?= /opt/rocm
PGO_SRC := pgo_check.cpp $(CSRC)/pgo.cpp $(CSRC)/pgo_kernels.hip $(CSRC)/map.cpp $(CSRC)/common.cpp
PGO_DEPS := $(PGO_SRC) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/rspl.h
PGO_FLAGS := -std=c++17 -O1 -Wall -Wno-unused-result -Wno-unused-variable --offload-arch=gfx950 -I$(CSRC)
PGO_LINK := -L$(PKG) -lrspl -Wl,-rpath,$(PKG)
HIP_SAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
           -Xarch_host -fno-omit-frame-pointer -g

pgo_check: build/pgo_check
build/pgo_check: pgo_check.cpp $(ROOT)/include/rspl.h $(PKG)/librspl.so
	mkdir -p build
	$(ROCM)/bin/hipcc $(PGO_FLAGS) -o $@ pgo_check.cpp $(PGO_LINK)

pgo_check_san: build/pgo_check_san
build/pgo_check_san: $(PGO_DEPS) $(PKG)/librspl.so
	mkdir -p build
	$(ROCM)/bin/hipcc $(PGO_FLAGS) $(HIP_SAN) -o $@ $(PGO_SRC) $(PGO_LINK)

.PHONY: pgo_check pgo_check_san
