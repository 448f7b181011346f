# Builds spt_guide_light_check (TEST INFRASTRUCTURE ONLY): the light guide's CPU resolve and shade under
# the host sanitizers, as a stand-alone program (tests/test_guide_light_host.py runs it; CPU only, never
# loaded into Python). The compiler and the flags are those of guide_check.mk.
#   make -C tests/probe -f guide_light_check.mk
HOSTCXX  ?= /opt/rocm/lib/llvm/bin/clang++
CSRC     := ../../small-pathtracer_amd/csrc
LIGHTCHECK    := spt_guide_light_check
LIGHTCHECKSRC := spt_guide_light_check.cpp $(CSRC)/spt_guide_light_host.cpp $(CSRC)/spt_dispatch.cpp \
                 $(CSRC)/spt_host.cpp
LIGHTCHECKHDR := $(CSRC)/spt_guide_light.h $(CSRC)/spt_film_math.h $(CSRC)/spt_window_shape.h \
                 $(CSRC)/spt_status.h $(CSRC)/spt_launch.h $(CSRC)/spt_variants.h $(CSRC)/spt_kparams.h \
                 $(CSRC)/spt_cornell.h $(CSRC)/spt_diag.h ../../include/spt.h

$(LIGHTCHECK): $(LIGHTCHECKSRC) $(LIGHTCHECKHDR) guide_light_check.mk
	$(HOSTCXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -o $@ $(LIGHTCHECKSRC)

clean:
	rm -f $(LIGHTCHECK)

.PHONY: clean
