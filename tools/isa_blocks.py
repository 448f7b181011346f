#!/usr/bin/env python3
"""Per-basic-block instruction mix of one kernel in a hipcc -S listing (static cost map).

  python tools/isa_blocks.py build/spt_kernel.s|build/spt_guide.s KEY [KEY2 ...] [--bb] [--min N]

The kernel is the one whose mangled name holds every KEY (an extern "C" kernel: whose name starts with
it), e.g. the Topo arguments and the Cfg arguments as two substrings. A key that fits several kernels is
an error: the candidates are listed and nothing is counted. const_nee, not a pixel-list kernel:
  TopoILi6ELi5ELi6ELb0ELi8ELb1ELin1ELin1ELin1ELb0ELb0ELin1ELb0ELb0E CfgILi1ELi0ELi1ELi1ELi1ELi1ELi1ELi1EEELb0E

--bb splits at LLVM's '; %bb.N' comments too (fall-through blocks), --min hides blocks with fewer
VALU. `slots` weights each VALU by its issue cost on gfx950 (tools/valu_rates.hip,
profiles/r01_valu_rates.txt, profiles/r21_valu_rates.txt, profiles/r22_valu_rates.txt): full-rate 1,
half-rate 2, transcendental 4. `far_sel` counts the VOP2 selects that do not directly follow their compare.
"""
import re
import sys
from collections import Counter

# Issue cost in VALU slots (one slot = a full-rate wave64 instruction, 2 cycles on a SIMD-32),
# measured by tools/valu_rates.hip (profiles/r01_valu_rates.txt): half-rate ops 2, transcendental 4.
# Round 21 (profiles/r21_valu_rates.txt) timed what the hot blocks are full of and found at half rate:
# the three-operand and the two-operand min / max (integer, and v_min_f32), the VOP3 select (an SGPR-pair mask), every
# compare, the carry add and mbcnt; v_lshl_add_u64 stays at half; v_fmaak / v_fmamk are full rate.
HALF = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_u32_u24",
        "v_mul_hi_u32_u24", "v_mad_u32_u24", "v_cvt_", "v_perm_b32", "v_bfe_", "v_bfi_b32",
        "v_add3_u32", "v_lshl_add_u32", "v_lshl_or_b32", "v_and_or_b32", "v_or3_b32", "v_med3_",
        "v_xad_u32", "v_pk_", "v_fma_f64", "v_add_f64", "v_mul_f64", "v_lshl_add_u64",
        "v_min3_", "v_max3_", "v_min_u32", "v_max_u32", "v_min_i32", "v_max_i32", "v_min_f32",
        "v_cndmask_b32_e64", "v_cmp_",
        "v_addc_co_u32", "v_mbcnt_")
QUARTER = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_", "v_exp_", "v_log_", "v_div_")
# Round 22 (profiles/r22_valu_rates.txt): v_ashrrev_i32, v_and_b32, v_sub_u32 and v_bitop3_b32 on three
# VGPRs are full rate; v_bitop3_b32 with an SGPR source is half rate (Philox's round keys), and so is
# v_subrev_co_u32 with the borrow in vcc or an SGPR pair. A VOP2 v_cndmask_b32 right behind the v_cmp
# that writes its vcc costs one slot (the pair reads 6.6 cycles, the compare alone 4.5). One that is not
# read 18 cycles in the probe, where all eight waves of a SIMD do the same: a wait of the wave, not an
# issue slot, so it stays at one slot here and is counted apart (`far_sel`).
HALF += ("v_subrev_co_u32",)
# Round 30 (profiles/r30_valu_rates.txt): v_alignbit_b32 is half rate (4.2 cycles), like v_bfe_i32 (4.3).
HALF += ("v_alignbit_b32",)
SGPR_SRC = re.compile(r"\bs(\d+|\[\d+:\d+\])")


def slots(op, args=""):
    if op.startswith(QUARTER):
        return 4
    if op.startswith(HALF):
        return 2
    if op == "v_bitop3_b32" and SGPR_SRC.search(args.split(",", 1)[-1]):
        return 2
    return 1


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_load") or op.startswith("s_buffer") or op == "s_memtime":
        return "smem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    return None


def find_kernel(lines, keys):
    """The line of the one kernel label that every key fits; SystemExit if none or several do."""
    if isinstance(keys, str):
        keys = [keys]
    found = []
    for i, l in enumerate(lines):
        if not re.match(r"^[A-Za-z_][\w$.]*:", l):
            continue
        name = l.split(":", 1)[0]
        # mangled kernels by substrings of the name, extern "C" ones by the start of it ("k_philox") or,
        # with a colon at the end, by the whole of it ("k_empty:")
        if (name.startswith("_Z") and all(k in name for k in keys)) or \
                (len(keys) == 1 and (name + ":").startswith(keys[0])):
            found.append((i, name))
    if len(found) != 1:
        what = "no kernel" if not found else f"{len(found)} kernels"
        raise SystemExit(f"isa_blocks: {what} for {' + '.join(keys)}" +
                         "".join(f"\n  {name}" for _, name in found))
    return found[0]


def blocks_of(path, key, bb=False):
    lines = open(path).read().splitlines()
    start, _ = find_kernel(lines, key)
    blocks, cur = [], None
    for n, l in enumerate(lines[start:]):
        if n == 0 and not l.startswith("_Z"):
            l = "_Z" + l  # an extern "C" entry label starts the first block like a mangled one
        s = l.strip()
        if s == "s_endpgm":
            break
        m = re.match(r"^(\.LBB[^:]+|_Z[^:]+):", s)
        m2 = re.match(r"^; (%bb\.\d+):", s) if bb else None
        if m or m2:
            cur = {"name": (m or m2).group(1)[:24], "valu": 0, "slots": 0, "salu": 0, "smem": 0,
                   "lds": 0, "vmem": 0, "wait": 0, "far_sel": 0, "ops": [], "vops": Counter()}
            blocks.append(cur)
            continue
        if not s or s.startswith((";", ".")) or cur is None:
            continue
        op = s.split()[0]
        c = classify(op)
        if c:
            cur[c] += 1
            if c == "valu":
                cur["slots"] += slots(op, s[len(op):].split(";")[0])
                cur["vops"][op] += 1
                # a VOP2 select whose vcc is not the instruction before's (see the rates above)
                prev = cur["ops"][-1] if cur["ops"] else ""
                if op == "v_cndmask_b32_e32" and not (prev.startswith("v_cmp") and prev.endswith("_e32")):
                    cur["far_sel"] += 1
            cur["ops"].append(op)
    return blocks


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path, key = args[0], args[1:]
    bb = "--bb" in sys.argv
    mn = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 0
    if "--min" in sys.argv:
        key = [k for k in key if k != sys.argv[sys.argv.index("--min") + 1]]
    blocks = blocks_of(path, key, bb)
    tot = {k: sum(b[k] for b in blocks) for k in ("valu", "slots", "salu", "smem", "lds", "vmem", "far_sel")}
    print("total", tot, "blocks", len(blocks))
    print("kernel", find_kernel(open(path).read().splitlines(), key)[1])
    for b in blocks:
        if b["valu"] < mn:
            continue
        br = [o for o in b["ops"] if o.startswith("s_cbranch") or o == "s_branch"]
        top = ", ".join(f"{k}:{v}" for k, v in b["vops"].most_common(4))
        print(f"{b['name']:24s} valu {b['valu']:4d} slots {b['slots']:4d} salu {b['salu']:3d} "
              f"smem {b['smem']:3d} lds {b['lds']:2d} vmem {b['vmem']:2d} far_sel {b['far_sel']:2d}  {' '.join(br)}  [{top}]")


if __name__ == "__main__":
    main()
