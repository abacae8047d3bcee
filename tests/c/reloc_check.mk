# reloc_check: rspl_lmap_debug_global_host, the host walk of the relocalisation contract (tests/c/reloc_check.cpp).
# It makes no device call, so it runs without a GPU.
#   make -C tests/c -f reloc_check.mk reloc_check       build/reloc_check: reloc_check.cpp linked with librspl's own
#                                                       objects of those sources (made through csrc/Makefile);
#                                                       tests/test_reloc_cpu.py builds and runs it
#   make -C tests/c -f reloc_check.mk reloc_check_san   build/reloc_check_san: the same sources with ASan + UBSan on
#                                                       the host code, on demand
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/rspl-slam_amd/csrc
ROCM ?= /opt/rocm
RELOC_SRC := reloc_check.cpp $(CSRC)/lmap_reloc.cpp $(CSRC)/lmap_global.hip $(CSRC)/common.cpp
RELOC_DEPS := $(RELOC_SRC) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/rspl.h
RELOC_FLAGS := -std=c++17 -O1 -Wall -Wno-unused-result --offload-arch=gfx950 -I$(CSRC)
HIP_SAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
           -Xarch_host -fno-omit-frame-pointer -g

RELOC_OBJ := build/lmap_reloc.o build/lmap_global.o build/common.o

reloc_check: build/reloc_check
csrc_objects:
	$(MAKE) -C $(CSRC) $(RELOC_OBJ)
build/reloc_check: reloc_check.cpp csrc_objects
	mkdir -p build
	$(ROCM)/bin/hipcc $(RELOC_FLAGS) -c -o build/reloc_check.o reloc_check.cpp
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -o $@ build/reloc_check.o $(addprefix $(CSRC)/,$(RELOC_OBJ))

reloc_check_san: build/reloc_check_san
build/reloc_check_san: $(RELOC_DEPS)
	mkdir -p build
	$(ROCM)/bin/hipcc $(RELOC_FLAGS) $(HIP_SAN) -o $@ $(RELOC_SRC)

.PHONY: reloc_check reloc_check_san csrc_objects
