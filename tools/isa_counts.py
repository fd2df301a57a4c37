"""Instruction counts of kernels in a gfx950 assembly listing (hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only of a
.hip file; no GPU needed).  usage: isa_counts.py <file.s> <substring of the demangled kernel name> [mnemonic prefix ...]
Prints, per matching kernel: instructions, the count of each mnemonic prefix, VGPRs, scratch bytes, and a SHA-256 of the
instruction stream (comments and directives stripped) so that two builds can be compared for equality."""
import hashlib
import re
import subprocess
import sys

PREFIXES = ["v_pk_fma", "v_readlane", "ds_read", "ds_write", "v_permlane32_swap", "scratch_"]


def kernels(path):
    """{mangled name: (instructions, {num_vgpr, private_seg_size})}"""
    out, name = {}, None
    for ln in open(path, errors="ignore"):
        if name is None:
            m = re.match(r"^(_Z\w+):\s*; @", ln)
            if m:
                name = m.group(1)
                out[name] = ([], {})
            else:
                m = re.match(r"^\s*\.set (_Z\w+)\.(num_vgpr|private_seg_size), (\d+)", ln)
                if m and m.group(1) in out:
                    out[m.group(1)][1][m.group(2)] = int(m.group(3))
            continue
        if ln.startswith(".Lfunc_end"):
            name = None
            continue
        s = ln.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out[name][0].append(re.sub(r"\s+", " ", s))
    return out


def main():
    path, want = sys.argv[1], sys.argv[2]
    prefixes = sys.argv[3:] or PREFIXES
    ks = kernels(path)
    names = list(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for mangled, pretty in zip(names, dem):
        if want not in pretty:
            continue
        instr, meta = ks[mangled]
        counts = "  ".join(f"{p} {sum(1 for i in instr if i.startswith(p))}" for p in prefixes)
        sha = hashlib.sha256("\n".join(instr).encode()).hexdigest()[:12]
        print(f"{pretty.split('(')[0].replace('void ', '')}\n    instr {len(instr)}  {counts}  VGPRs {meta.get('num_vgpr', '?')}  "
              f"scratch {meta.get('private_seg_size', '?')}  stream {sha}")


if __name__ == "__main__":
    main()
