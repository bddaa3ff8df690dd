"""Kernel-by-kernel comparison of two sets of gfx950 assembly files (developer tool, the
gate of a refactor that must not change compiled kernels):

    python tools/isa_compare.py OLD_DIR NEW_DIR > profiles/<name>_isa.txt

Every *.s under the two directories (hipcc ... --cuda-device-only -S) is cut into its
kernels.  A kernel's instruction sequence is its body without comments, directives,
debug lines and local label numbers, with its own mangled name replaced.  Kernels are
matched by mangled name and template arguments (attention_x3_kernel's without the
parameters that its refactor made constants); a pair prints "identical", or the counts that the
gate reads: instructions, MFMA, s_waitcnt, s_barrier, v_mov*, and the metadata's VGPRs,
AGPRs, spills and scratch bytes.
"""
import re
import sys
from pathlib import Path


def kernels(path):
    txt = Path(path).read_text()
    meta = {}
    for rec in re.split(r"\n  - ", txt[txt.find("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        if "name" in f and "\n" + f["name"] + ":" in txt:
            meta[f["name"]] = f
    out = {}
    for name, f in meta.items():
        start = txt.index("\n", txt.index("\n" + name + ":") + 1)
        body = txt[start:txt.index(".Lfunc_end", start)]
        seq = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith((".loc", ".file", ".cfi", ".p2align", ".section")):
                continue
            line = re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", line).replace(name, "KERNEL")
            seq.append(re.sub(r"\s+", " ", line))
        out[name] = (seq, f)
    return out


def key_of(mangled):
    """The kernel's name and template arguments as mangled (the parameter list cut off),
    without bool arguments, and with attention_x3's former tile-count argument dropped."""
    k = mangled[:mangled.index("EEv") + 2] if "EEv" in mangled else mangled
    if "attention_x3_kernel" in k:
        k = re.sub(r"Lb[01]E", "", k).replace("Li3ELi", "Li")
    return k


def counts(seq, f):
    ins = [s for s in seq if not s.endswith(":")]
    n = lambda pat: sum(1 for s in ins if re.match(pat, s))
    return (f"instr {len(ins)} mfma {n('v_mfma')} s_waitcnt {n('s_waitcnt')} s_barrier "
            f"{n('s_barrier')} v_mov {n('v_mov')} | vgpr {f.get('vgpr_count')} agpr "
            f"{f.get('agpr_count')} spill {f.get('vgpr_spill_count')} scratch "
            f"{f.get('private_segment_fixed_size')}")


def load(d):
    ks = {}
    for p in sorted(Path(d).glob("*.s")):
        for name, v in kernels(p).items():
            ks[key_of(name)] = (p.name,) + v
    return ks


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print(f"{k}: only in OLD ({old[k][0]})  {counts(*old[k][1:])}")
        elif k not in old:
            print(f"{k}: only in NEW ({new[k][0]})  {counts(*new[k][1:])}")
        elif old[k][1] == new[k][1]:
            print(f"{k}: identical ({old[k][0]} -> {new[k][0]})  {counts(*new[k][1:])}")
        else:
            print(f"{k}: DIFFERS ({old[k][0]} -> {new[k][0]})\n    old {counts(*old[k][1:])}\n"
                  f"    new {counts(*new[k][1:])}")


if __name__ == "__main__":
    main()
