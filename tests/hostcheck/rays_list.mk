# A ray accumulator's list pass on the host — TEST INFRASTRUCTURE (see
# pt_rays_list_host.cpp), with the hostcheck Makefile's g++ flags.
#   make -f rays_list.mk [BUILD=dir]: dir/librayslist.so (default: build/),
#   loaded by tests/test_rays_adaptive_host.py, which builds it into a
#   temporary directory
CXX ?= g++
BUILD := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))build
CSRC := ../../pathtracerpython_amd/csrc
DEPS := $(CSRC)/pt_core.h $(CSRC)/pt_path.h $(CSRC)/pt_wavefront.h $(CSRC)/pt_prepare.h $(CSRC)/pt_job.h \
        $(CSRC)/pt_plan.h ../../include/pt_capi.h ../devcheck/filter_eval.h
rays_list: $(BUILD)/librayslist.so
$(BUILD)/librayslist.so: pt_rays_list_host.cpp pt_rays_host.cpp pt_lens_host.cpp pt_aa_host.cpp pt_hostcheck.cpp \
        $(DEPS) rays_list.mk
	@mkdir -p $(BUILD)
	$(CXX) -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Wall -Wno-unknown-pragmas -o $@ pt_rays_list_host.cpp
.PHONY: rays_list
