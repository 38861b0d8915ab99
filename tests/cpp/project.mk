# TEST PROGRAM: project_cpp, the BICOS::project driver of tests/test_project_cpp.py
# (links the in-tree libbicos_amd.so):  make -C tests/cpp -f project.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
project_cpp: project_cpp.cpp $(ROOT)/include/bicos/project.hpp $(ROOT)/include/bicos/common.hpp \
             $(ROOT)/include/bicos/types.hpp $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f project_cpp
.PHONY: clean
