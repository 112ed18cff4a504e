"""How much of k_gumbel_search's network code the compiler lays out differently between two forms of the select phase
(csrc/search.hip, template argument PARTS) -- a compile-time check, no GPU.

    python profiles/mfma_loop_diff.py 6                      # the default form against form 0
    python profiles/mfma_loop_diff.py 4 -DSOME_VARIANT       # MUZ_SELECT_PARTS=4 with further flags
    python profiles/mfma_loop_diff.py ring                   # the default form's two weight addressings (nn.hpp SB)

Compiles search.hip's device code to assembly with MUZ_SELECT_PARTS=m, takes the opcode streams (operands dropped) of
k_gumbel_search<0> and k_gumbel_search<m>, and counts the differing hunks that touch an MFMA, a 128-bit LDS read or a
128-bit global load, i.e. the dense layers' loops.  A change of the select phase that leaves this at (nearly) 0 runs the
networks on the same schedule as before; one that does not has to be measured as a change of the whole kernel
(profiles/select_invariants_ab.log: a plain table read in the walk changed 166 hunks and cost 0.5-0.8 % per launch).

`ring` compares k_gumbel_search<default, SB = false> with <default, SB = true> instead and also prints, for each, the
counts of the opcodes the addressing is about (profiles/ring_addressing_ab.log)."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "exploring-muzero-on-dog_amd", "csrc", "search.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOT = ("mfma", "ds_read_b128", "dwordx4")


def opcodes(path):
    """{(PARTS, SB): [opcode, ...]} of every k_gumbel_search instantiation in an assembly file; a load in the
    scalar-base form (v_off, s[base:base+1]) is listed as global_load_dwordx4_saddr."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^_ZN3muz15k_gumbel_searchILi(\d+)ELb([01])EE\S*:", line)
        if m:
            cur = (m.group(1), m.group(2))
            out[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            t = line.strip()
            if t and not t.startswith((";", ".")):
                op = t.split()[0]
                if op.startswith("global_load") and re.search(r", s\[\d+:\d+\]", t):
                    op += "_saddr"
                out[cur].append(op)
    return out


def main():
    m, extra = sys.argv[1], sys.argv[2:]
    ring = m == "ring"
    if ring:
        m = "6"
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "search.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-w",
                        f"-DMUZ_SELECT_PARTS={m}", *extra, "-S", "--cuda-device-only", SRC, "-o", asm], check=True)
        fs = opcodes(asm)
    x, y = (fs[(m, "0")], fs[(m, "1")]) if ring else (fs[("0", "1")], fs[(m, "1")])
    if ring:
        ops = ("v_mfma_f32_16x16x4_f32", "global_load_dwordx4", "global_load_dwordx4_saddr", "v_lshl_add_u64",
               "v_add_co_u32_e32", "v_addc_co_u32_e32", "v_addc_co_u32_e64", "s_add_u32", "s_addc_u32",
               "v_readfirstlane_b32", "s_nop", "s_waitcnt")
        for name, f in (("SB=0", x), ("SB=1", y)):
            c = collections.Counter(f)
            print(f"{name}: {len(f)} instructions; " + ", ".join(f"{o} {c[o]}" for o in ops))
    hunks = changed = 0
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes():
        if tag != "equal" and any(h in op for op in x[i1:i2] + y[j1:j2] for h in HOT):
            hunks += 1
            changed += (i2 - i1) + (j2 - j1)
    print(f"{'ring, ' if ring else ''}parts {m} {' '.join(extra)}: {len(x)} -> {len(y)} instructions; dense-loop hunks changed {hunks} "
          f"({changed} instructions)")


if __name__ == "__main__":
    main()
