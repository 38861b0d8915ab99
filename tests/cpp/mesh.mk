# TEST PROGRAM: mesh_cpp, the BICOS::mesh driver of tests/test_mesh_cpp.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f mesh.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
mesh_cpp: mesh_cpp.cpp $(ROOT)/include/bicos/mesh.hpp $(ROOT)/include/bicos/reproject.hpp \
          $(ROOT)/include/bicos/common.hpp $(ROOT)/include/bicos/types.hpp \
          $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f mesh_cpp
.PHONY: clean
