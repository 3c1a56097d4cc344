"""Per-kernel resources of a built tree, from the code-object metadata: VGPRs, AGPRs, SGPRs, spills,
scratch, static LDS and kernel-argument bytes of every kernel in csrc/build/*.o (no GPU needed).

    python tools/kernel_resources.py [TREE]              # one JSON object: symbol -> figures
    python tools/kernel_resources.py TREE_A TREE_B       # what differs between two built trees

The second form is the check that a change left the training step's kernels alone: every symbol
of TREE_A must exist in TREE_B with the same figures; differences and new symbols are listed.
Uses the ROCm LLVM tools next to hipcc (llvm-objcopy, clang-offload-bundler, llvm-readelf).
"""
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def _llvm(tool):
    from greedy_multimodal_learning_amd.build import ARCH, hipcc
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin"), os.path.dirname(hipcc())):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool), ARCH
    raise RuntimeError(f"{tool} not found near {hipcc()}")


def resources(tree):
    objs = sorted(glob.glob(os.path.join(tree, "greedy_multimodal_learning_amd", "csrc", "build", "*.o")))
    if not objs:
        raise RuntimeError(f"{tree}: no objects under csrc/build (build the tree first)")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
            objcopy, arch = _llvm("llvm-objcopy")
            if subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fb, o], capture_output=True).returncode:
                continue  # (an object without device code)
            subprocess.run([_llvm("clang-offload-bundler")[0], "--unbundle", "--type=o",
                            f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", "--input=" + fb, "--output=" + co],
                           check=True)
            notes = subprocess.run([_llvm("llvm-readelf")[0], "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
                blk = ".agpr_count:" + blk
                name = re.search(r"\.name:\s*(\S+)", blk).group(1)
                out[name] = {k[1:]: int(m.group(1)) if (m := re.search(re.escape(k) + r":\s*(\d+)", blk)) else None
                             for k in KEYS}
    return out


def main():
    trees = sys.argv[1:] or [ROOT]
    if len(trees) == 1:
        print(json.dumps(resources(trees[0]), indent=1, sort_keys=True))
        return 0
    a, b = resources(trees[0]), resources(trees[1])
    bad = 0
    for name in sorted(a):
        if name not in b:
            print(f"MISSING {name}")
            bad += 1
        elif a[name] != b[name]:
            diff = {k: (a[name][k], b[name][k]) for k in a[name] if a[name][k] != b[name][k]}
            print(f"DIFF {name}: {diff}")
            bad += set(diff) != {"kernarg_segment_size"}
    for name in sorted(set(b) - set(a)):
        print(f"NEW {name}: {b[name]}")
    print(f"{len(a)} kernels in {trees[0]}, {len(b)} in {trees[1]}; {bad} differ in more than the argument bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
