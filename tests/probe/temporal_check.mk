# Builds spt_temporal_check (TEST INFRASTRUCTURE ONLY): temporal accumulation's CPU statement under the
# host sanitizers, as a stand-alone program (tests/test_temporal_host.py runs it; CPU only, never loaded
# into Python). The compiler and the flags are those of guide_check.mk.
#   make -C tests/probe -f temporal_check.mk
HOSTCXX  ?= /opt/rocm/lib/llvm/bin/clang++
CSRC     := ../../small-pathtracer_amd/csrc
TPCHECK    := spt_temporal_check
TPCHECKSRC := spt_temporal_check.cpp $(CSRC)/spt_temporal_host.cpp $(CSRC)/spt_dispatch.cpp $(CSRC)/spt_host.cpp
TPCHECKHDR := $(CSRC)/spt_temporal.h $(CSRC)/spt_denoise.h $(CSRC)/spt_film_math.h $(CSRC)/spt_status.h \
              $(CSRC)/spt_launch.h $(CSRC)/spt_variants.h $(CSRC)/spt_kparams.h $(CSRC)/spt_cornell.h \
              $(CSRC)/spt_diag.h ../../include/spt.h

$(TPCHECK): $(TPCHECKSRC) $(TPCHECKHDR) temporal_check.mk
	$(HOSTCXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -o $@ $(TPCHECKSRC)

clean:
	rm -f $(TPCHECK)

.PHONY: clean
