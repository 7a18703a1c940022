# tests/cpp/test_sptrsv_api.cpp — sparse::SpTRSVPlan / sparse::sptrsv of
# sparse/SpTRSV.hpp — built with the flags tests/cpp/Makefile gives
# test_cpp_api (headers from include/, linked against the in-tree liblhpc.so
# and the HIP runtime):
#   make -C tests/cpp -f sptrsv.mk
# Run by __graft_entry__.build() and tests/test_sptrsv_api.py; the program
# runs on the GPU in tests/test_gpu_sptrsv.py.
#   make -C tests/cpp -f sptrsv.mk asan
# builds tests/cpp/asan_sptrsv.cpp with the solve's host analysis
# (libhpc_amd/csrc/lhpc_sptrsv_host.cpp, no HIP) under ASan/UBSan: a
# stand-alone CPU program, run by tests/test_sptrsv_asan.py.
CXX ?= g++
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/libhpc_amd/_lib
ROCM ?= /opt/rocm
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -fopenmp -I$(ROOT)/include -I$(ROOT)/include/hpc \
           -I$(ROOT)/include/sparse
HIPCXX = -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include
HIPLIB = -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib
HDRS = $(wildcard $(ROOT)/include/*.h* $(ROOT)/include/*/*.hpp)
RPATH = -Wl,-rpath,'$$ORIGIN/../../../libhpc_amd/_lib'
SAN = -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g
CSRC = $(ROOT)/libhpc_amd/csrc

all: _build/test_sptrsv_api

_build/test_sptrsv_api: test_sptrsv_api.cpp $(HDRS) $(LIBDIR)/liblhpc.so
	mkdir -p _build
	$(CXX) $(CXXFLAGS) $(HIPCXX) test_sptrsv_api.cpp -o $@ -L$(LIBDIR) -llhpc $(RPATH) $(HIPLIB)

asan: _build/asan/asan_sptrsv

_build/asan/asan_sptrsv: asan_sptrsv.cpp $(CSRC)/lhpc_sptrsv_host.cpp $(CSRC)/lhpc_sptrsv.hpp $(HDRS)
	mkdir -p _build/asan
	$(CXX) $(CXXFLAGS) $(SAN) asan_sptrsv.cpp $(CSRC)/lhpc_sptrsv_host.cpp -o $@

.PHONY: all asan
