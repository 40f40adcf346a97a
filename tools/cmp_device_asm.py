"""Are the kernels of two device assembly files (hipcc -S --cuda-device-only, e.g. wdpm_amd/csrc/build/wdpm_march.s of two revisions)
the same code?  Per .amdhsa_kernel symbol the instruction text and the kernel descriptor (.amdhsa_*: VGPRs, SGPRs, LDS, scratch) must
be identical.  Functions are emitted in the order of first use, so their order and the function numbers inside local labels
(.LBB<n>_, .Lfunc_end<n>, .Lpost_getpc<n>) differ after a host-side change: those, and the comments that quote them, are normalised away.
usage: python3 tools/cmp_device_asm.py a.s b.s      (exit status 1 when a kernel differs)"""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}

    def norm(s):
        s = re.sub(r"\s*;.*$", "", s, flags=re.M)                      # comments (loop headers quote label numbers)
        s = re.sub(r"BB\d+_", "BB_", s)
        return re.sub(r"\.L(func_end|post_getpc)\d+", r".L\1", s)
    for m in re.finditer(r"(?ms)^(_Z\w+|\w+_kernel\w*):\s*;.*?^\.Lfunc_end\d+:", text):
        out[m.group(1)] = [norm(m.group(0))]
    for m in re.finditer(r"(?ms)^\s*\.amdhsa_kernel\s+(\S+)\n.*?\.end_amdhsa_kernel", text):
        out.setdefault(m.group(1), [None]).append(norm(m.group(0)))
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(f"{len(a)} / {len(b)} kernels, same symbols: {set(a) == set(b)}, differing: {len(bad)}")
    for k in bad:
        print(" ", k)
    sys.exit(1 if bad else 0)
