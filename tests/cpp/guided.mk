# TEST PROGRAM: guided_cpp, the BICOS::guide_from_disparity / guided BICOS::match driver of
# tests/test_guided_cpp.py (links the in-tree libbicos_amd.so):  make -C tests/cpp -f guided.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
guided_cpp: guided_cpp.cpp $(ROOT)/include/bicos/guide.hpp $(ROOT)/include/bicos/match.hpp \
            $(ROOT)/include/bicos/common.hpp $(ROOT)/include/bicos/types.hpp \
            $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(ROOT)/libbicos_amd -lbicos_amd \
	    -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f guided_cpp
.PHONY: clean
