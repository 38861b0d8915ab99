# TEST PROGRAM: transform_pk_check, the packed LIMITED transform's integer arithmetic alone
# (libbicos_amd/csrc/transform_pk.hpp; host only, links nothing) for tests/test_transform_pk.py,
# and the same program once more under the address and undefined-behaviour sanitizers:
#   make -C tests/cpp -f transform_pk.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../libbicos_amd/csrc
all: transform_pk_check transform_pk_check_san
transform_pk_check: transform_pk_check.cpp $(CSRC)/transform_pk.hpp
	$(HIPCC) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@
transform_pk_check_san: transform_pk_check.cpp $(CSRC)/transform_pk.hpp
	$(HIPCC) -O1 -g -std=c++17 -Wall -Xarch_host -fsanitize=address,undefined \
	    -Xarch_host -fno-sanitize-recover=undefined -I$(CSRC) $< -o $@
clean:
	rm -f transform_pk_check transform_pk_check_san
.PHONY: all clean
