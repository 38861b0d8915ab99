# TEST PROGRAM: normals_cpp, the BICOS::normals driver of tests/test_normals_cpp.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f normals.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
normals_cpp: normals_cpp.cpp $(ROOT)/include/bicos/normals.hpp $(ROOT)/include/bicos/reproject.hpp \
             $(ROOT)/include/bicos/common.hpp $(ROOT)/include/bicos/types.hpp \
             $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f normals_cpp
.PHONY: clean
