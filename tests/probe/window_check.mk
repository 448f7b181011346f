# Builds spt_window_check (TEST INFRASTRUCTURE ONLY): what a film and a guide share (spt_window_shape.h)
# under the host sanitizers, as a stand-alone program (tests/test_window_shape_host.py runs it; CPU
# only, never loaded into Python). The compiler and the flags are those of Makefile's spt_film_check rule.
#   make -C tests/probe -f window_check.mk
HOSTCXX  ?= /opt/rocm/lib/llvm/bin/clang++
CSRC     := ../../small-pathtracer_amd/csrc
WINDOWCHECK    := spt_window_check
WINDOWCHECKSRC := spt_window_check.cpp $(CSRC)/spt_dispatch.cpp $(CSRC)/spt_host.cpp
WINDOWCHECKHDR := $(CSRC)/spt_window_shape.h $(CSRC)/spt_status.h $(CSRC)/spt_launch.h $(CSRC)/spt_variants.h \
                  $(CSRC)/spt_kparams.h $(CSRC)/spt_cornell.h $(CSRC)/spt_diag.h ../../include/spt.h

$(WINDOWCHECK): $(WINDOWCHECKSRC) $(WINDOWCHECKHDR) window_check.mk
	$(HOSTCXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -o $@ $(WINDOWCHECKSRC)

clean:
	rm -f $(WINDOWCHECK)

.PHONY: clean
