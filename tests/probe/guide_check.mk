# Builds spt_guide_check (TEST INFRASTRUCTURE ONLY): the guide's CPU resolve under the host
# sanitizers, as a stand-alone program (tests/test_guide_host.py runs it; CPU only, never loaded into
# Python). The compiler and the flags are those of Makefile's spt_film_check rule.
#   make -C tests/probe -f guide_check.mk
HOSTCXX  ?= /opt/rocm/lib/llvm/bin/clang++
CSRC     := ../../small-pathtracer_amd/csrc
GUIDECHECK    := spt_guide_check
GUIDECHECKSRC := spt_guide_check.cpp $(CSRC)/spt_guide_host.cpp $(CSRC)/spt_dispatch.cpp $(CSRC)/spt_host.cpp
GUIDECHECKHDR := $(CSRC)/spt_guide.h $(CSRC)/spt_film_math.h $(CSRC)/spt_launch.h $(CSRC)/spt_variants.h \
                 $(CSRC)/spt_kparams.h $(CSRC)/spt_cornell.h $(CSRC)/spt_diag.h ../../include/spt.h

$(GUIDECHECK): $(GUIDECHECKSRC) $(GUIDECHECKHDR) guide_check.mk
	$(HOSTCXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -o $@ $(GUIDECHECKSRC)

clean:
	rm -f $(GUIDECHECK)

.PHONY: clean
