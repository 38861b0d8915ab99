# TEST PROGRAM: median_cpp, the BICOS::median_filter driver of tests/test_median_gpu.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f median.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
median_cpp: median_cpp.cpp $(ROOT)/include/bicos/median.hpp $(ROOT)/include/bicos/common.hpp \
            $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f median_cpp
.PHONY: clean
