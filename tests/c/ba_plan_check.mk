# ba_plan_check: the local BA's host-only pieces -- the line-workgroup packing (csrc/ba_stage.cpp) and the window
# plan (csrc/ba_plan.cpp) -- from C++ (tests/c/ba_plan_check.cpp).  It makes no device call, so it runs without a GPU.
# The plan asks ba_schur.hip for wave_path and ba_trial.hip for set_update_geometry (two host functions beside the
# kernels): both targets link librspl's own objects of those two files (made through csrc/Makefile).
#   make -C tests/c -f ba_plan_check.mk ba_plan_check       build/ba_plan_check: ba_plan_check.cpp linked with librspl's
#                                                           own objects; tests/test_ba_plan_check_cpu.py builds and runs it
#   make -C tests/c -f ba_plan_check.mk ba_plan_check_san   build/ba_plan_check_san: ba_plan_check.cpp, ba_plan.cpp,
#                                                           ba_stage.cpp and common.cpp under ASan + UBSan (host code)
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
CSRC := $(ROOT)/rspl-slam_amd/csrc
ROCM ?= /opt/rocm
PLAN_SRC := ba_plan_check.cpp $(CSRC)/ba_plan.cpp $(CSRC)/ba_stage.cpp $(CSRC)/common.cpp
PLAN_DEPS := $(PLAN_SRC) $(wildcard $(CSRC)/*.hpp) $(ROOT)/include/rspl.h
PLAN_FLAGS := -std=c++17 -O1 -Wall -Wno-unused-result --offload-arch=gfx950 -I$(CSRC)
HIP_SAN := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
           -Xarch_host -fno-omit-frame-pointer -g

KERNEL_OBJ := build/ba_schur.o build/ba_trial.o
PLAN_OBJ := build/ba_plan.o build/ba_stage.o build/common.o $(KERNEL_OBJ)

ba_plan_check: build/ba_plan_check
csrc_objects:
	$(MAKE) -C $(CSRC) $(PLAN_OBJ)
build/ba_plan_check: ba_plan_check.cpp csrc_objects
	mkdir -p build
	$(ROCM)/bin/hipcc $(PLAN_FLAGS) -c -o build/ba_plan_check.o ba_plan_check.cpp
	$(ROCM)/bin/hipcc --offload-arch=gfx950 -o $@ build/ba_plan_check.o $(addprefix $(CSRC)/,$(PLAN_OBJ))

ba_plan_check_san: build/ba_plan_check_san
build/ba_plan_check_san: $(PLAN_DEPS) | csrc_objects
	mkdir -p build/ba_plan_san
	for s in $(PLAN_SRC); do \
	  $(ROCM)/bin/hipcc $(PLAN_FLAGS) $(HIP_SAN) -c -o build/ba_plan_san/$$(basename $$s .cpp).o $$s || exit 1; done
	$(ROCM)/bin/hipcc --offload-arch=gfx950 $(HIP_SAN) -o $@ \
	  $(patsubst %.cpp,build/ba_plan_san/%.o,$(notdir $(PLAN_SRC))) $(addprefix $(CSRC)/,$(KERNEL_OBJ))

.PHONY: ba_plan_check ba_plan_check_san csrc_objects
