# Builds spt_denoise_bank_check (TEST INFRASTRUCTURE ONLY): the filter bank's CPU statement and its
# summary under the host sanitizers, as a stand-alone program (tests/test_denoise_bank_host.py runs it;
# CPU only, never loaded into Python). The compiler and the flags are those of denoise_check.mk.
#   make -C tests/probe -f denoise_bank_check.mk
HOSTCXX  ?= /opt/rocm/lib/llvm/bin/clang++
CSRC     := ../../small-pathtracer_amd/csrc
DBCHECK    := spt_denoise_bank_check
DBCHECKSRC := spt_denoise_bank_check.cpp $(CSRC)/spt_denoise_host.cpp $(CSRC)/spt_dispatch.cpp $(CSRC)/spt_host.cpp
DBCHECKHDR := $(CSRC)/spt_denoise.h $(CSRC)/spt_film_math.h $(CSRC)/spt_launch.h $(CSRC)/spt_variants.h \
              $(CSRC)/spt_kparams.h $(CSRC)/spt_cornell.h $(CSRC)/spt_diag.h ../../include/spt.h

$(DBCHECK): $(DBCHECKSRC) $(DBCHECKHDR) denoise_bank_check.mk
	$(HOSTCXX) -O1 -g -std=c++17 -ffp-contract=off -Wall -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -o $@ $(DBCHECKSRC)

clean:
	rm -f $(DBCHECK)

.PHONY: clean
