# tests/native/div.mk — the short division sequences' GPU test helper (tests/test_gpu_division.py).
HIPCC ?= /opt/rocm/bin/hipcc
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../qt-raytracer_amd/csrc
# the product's arithmetic flags (qt-raytracer_amd/Makefile)
FLAGS := --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -I$(CSRC) -I$(HERE)../../include

all: $(HERE)libdiv_selftest.so

$(HERE)libdiv_selftest.so: $(HERE)div_selftest.hip $(CSRC)/hippt_trace.h
	$(HIPCC) $(FLAGS) -shared -o $@ $<

.PHONY: all
