# TEST PROGRAM: pool_cpp, the BICOS::pool_stack / BICOS::match_pyramid driver of
# tests/test_pool_cpp.py (links the in-tree libbicos_amd.so):  make -C tests/cpp -f pool.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
pool_cpp: pool_cpp.cpp $(ROOT)/include/bicos/pool.hpp $(ROOT)/include/bicos/common.hpp \
          $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f pool_cpp
.PHONY: clean
