# TEST PROGRAM: ply_color_check, bicos_cli::write_ply_colored alone (tests/test_project_api.py;
# host only, as imageio_check it links the in-tree libbicos_amd.so for BICOS::Image):
#   make -C tests/cpp -f ply_color.mk
HIPCC ?= /opt/rocm/bin/hipcc
ROOT = ../..
ply_color_check: ply_color_check.cpp $(ROOT)/libbicos_amd/cli/imageio.cpp $(ROOT)/libbicos_amd/cli/imageio.hpp \
           $(ROOT)/libbicos_amd/libbicos_amd.so
	$(HIPCC) -O2 -std=c++17 -Wall -I$(ROOT)/include $< $(ROOT)/libbicos_amd/cli/imageio.cpp \
	    -L$(ROOT)/libbicos_amd -lbicos_amd -lz -Wl,-rpath,'$$ORIGIN/../../libbicos_amd' -o $@
clean:
	rm -f ply_color_check
.PHONY: clean
