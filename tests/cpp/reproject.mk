# TEST PROGRAM: reproject_cpp, the BICOS::reproject driver of tests/test_reproject_gpu.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f reproject.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
reproject_cpp: reproject_cpp.cpp $(ROOT)/include/bicos/reproject.hpp $(ROOT)/include/bicos/common.hpp \
               $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f reproject_cpp
.PHONY: clean
