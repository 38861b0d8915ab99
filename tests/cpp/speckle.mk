# TEST PROGRAM: speckle_cpp, the BICOS::filter_speckles driver of tests/test_speckle_gpu.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f speckle.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
speckle_cpp: speckle_cpp.cpp $(ROOT)/include/bicos/speckle.hpp $(ROOT)/include/bicos/common.hpp \
             $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f speckle_cpp
.PHONY: clean
