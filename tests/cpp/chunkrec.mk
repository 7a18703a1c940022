# tests/cpp/chunkrec_plan.cpp — the XTILE chunk-record builder and its policy,
# host code only (lhpc_plan.cpp and lhpc_gen.cpp compiled in), with the
# sanitizer flags tests/cpp/Makefile gives asan_plan:
#   make -C tests/cpp -f chunkrec.mk
# Built and run by tests/test_chunkrec_plan.py.
CXX ?= g++
ROOT := $(abspath ../..)
CSRC = $(ROOT)/libhpc_amd/csrc
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -fopenmp -I$(ROOT)/include
SAN = -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -g

all: _build/asan/chunkrec_plan

_build/asan/chunkrec_plan: chunkrec_plan.cpp $(CSRC)/lhpc_plan.cpp $(CSRC)/lhpc_gen.cpp $(CSRC)/lhpc_plan.hpp $(ROOT)/include/lhpc.h
	mkdir -p _build/asan
	$(CXX) $(CXXFLAGS) $(SAN) chunkrec_plan.cpp $(CSRC)/lhpc_plan.cpp $(CSRC)/lhpc_gen.cpp -o $@

.PHONY: all
