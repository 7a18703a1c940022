# tests/cpp/test_bicgstab_api.cpp — sparse::bicgstab of sparse/SpMV.hpp — built
# with the flags tests/cpp/Makefile gives test_cpp_api (headers from include/,
# linked against the in-tree liblhpc.so and the HIP runtime):
#   make -C tests/cpp -f bicgstab.mk
# Run by __graft_entry__.build() and tests/test_bicgstab_api.py; the program
# runs on the GPU in tests/test_gpu_bicgstab.py.
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

all: _build/test_bicgstab_api

_build/test_bicgstab_api: test_bicgstab_api.cpp $(HDRS) $(LIBDIR)/liblhpc.so
	mkdir -p _build
	$(CXX) $(CXXFLAGS) $(HIPCXX) test_bicgstab_api.cpp -o $@ -L$(LIBDIR) -llhpc $(RPATH) $(HIPLIB)

.PHONY: all
