# TEST PROGRAM: rectify_cpp, the BICOS::rectify / BICOS::rectify_maps driver of
# tests/test_rectify_gpu.py (links the in-tree libbicos_amd.so):  make -C tests/cpp -f rectify.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
rectify_cpp: rectify_cpp.cpp $(ROOT)/include/bicos/rectify.hpp $(ROOT)/include/bicos/common.hpp \
             $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f rectify_cpp
.PHONY: clean
