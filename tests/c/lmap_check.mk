# lmap_check: csrc/lmap.cpp's bank / local-table bookkeeping on a host-only handle and the host instantiation of
# csrc/lmap_match.hpp (tests/c/lmap_check.cpp).  hipcc over the handle's own sources, the tracker calls stubbed; it
# makes no device call, so it runs without a GPU.
#   make -C tests/c -f lmap_check.mk lmap_check       build/lmap_check: lmap_check.cpp linked with librspl's own
#                                                     objects of those sources (made through csrc/Makefile);
#                                                     tests/test_lmap_cpu.py builds and runs it
#   make -C tests/c -f lmap_check.mk lmap_check_san   build/lmap_check_san: the sources compiled again with ASan +
#                                                     UBSan on the host code, on demand
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/rspl-slam_amd/csrc
ROCM ?= /opt/rocm
LMAP_SRC := lmap_check.cpp $(CSRC)/lmap.cpp $(CSRC)/lmap_kernels.hip $(CSRC)/copy_kernels.hip $(CSRC)/common.cpp
LMAP_DEPS := $(LMAP_SRC) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/rspl.h
LMAP_FLAGS := -std=c++17 -O1 -Wall -Wno-unused-result --offload-arch=gfx950 -I$(CSRC)
HIP_SAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
           -Xarch_host -fno-omit-frame-pointer -g

LMAP_OBJ := build/lmap.o build/lmap_kernels.o build/copy_kernels.o build/common.o

lmap_check: build/lmap_check
csrc_objects:
	$(MAKE) -C $(CSRC) $(LMAP_OBJ)
build/lmap_check: lmap_check.cpp csrc_objects
	mkdir -p build
	$(ROCM)/bin/hipcc $(LMAP_FLAGS) -c -o build/lmap_check.o lmap_check.cpp
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -o $@ build/lmap_check.o $(addprefix $(CSRC)/,$(LMAP_OBJ))

lmap_check_san: build/lmap_check_san
build/lmap_check_san: $(LMAP_DEPS)
	mkdir -p build
	$(ROCM)/bin/hipcc $(LMAP_FLAGS) $(HIP_SAN) -o $@ $(LMAP_SRC)

.PHONY: lmap_check lmap_check_san csrc_objects
