#!/usr/bin/env python3
"""Registers, spills and scratch of every kernel in hipcc objects, from the code-object metadata (no GPU needed).

    tools/kernel_resources.py DIR_OR_OBJECT...            one line per kernel
    tools/kernel_resources.py --diff BASE_DIR NEW_DIR [STRIP]
                                                          kernels whose figures differ between two builds, and every kernel that
                                                          gained a spill or scratch (exit status 1 then).  STRIP: a regular
                                                          expression for the pieces of the mangled names to leave out when the
                                                          builds are matched (a parameter that one build added: PKNS_7FwFrameE)
    tools/kernel_resources.py --same-code BASE NEW        whether two builds hold the same device code: per object (directories are
                                                          matched by basename), the same kernel names and the same sha256 of the
                                                          code object's .text (not of the whole code object: its metadata names the
                                                          source file).  Where the builds hold different kernels (one of them
                                                          added instantiations to an object), the kernels present in both are
                                                          compared one by one, by the sha256 of each kernel's own bytes of .text,
                                                          and the others are listed, as is an object that only NEW has (new
                                                          kernels only).  Exit status 1 on a kernel or an object that differs, or
                                                          an object that only BASE has
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")


def kernels(obj, arch="gfx950", text=False):
    """{kernel name: (vgpr, agpr, sgpr, vgpr spills, sgpr spills, scratch bytes)} of one host object with an embedded code object;
    with text, the sha256 of the code object's .text and {kernel name: sha256 of its own bytes of .text} as well: (kernels, digest,
    per kernel)"""
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, "a.hipfb"), os.path.join(tmp, "a.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch,
                               "--input=" + fb, "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        if text:
            subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, os.path.join(tmp, "a.text")])
            with open(os.path.join(tmp, "a.text"), "rb") as f:
                code = f.read()
            digest = hashlib.sha256(code).hexdigest()
            sections = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co], text=True)
            base = int(re.search(r"\s\.text\s+PROGBITS\s+([0-9a-f]+)", sections).group(1), 16)
            per = {}
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co], text=True).splitlines():
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
                    at, size = int(f[1], 16) - base, int(f[2], 0)
                    per[f[7]] = hashlib.sha256(code[at:at + size]).hexdigest()
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "    - .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        vals = []
        for f in FIELDS:
            m = re.search(re.escape(f) + r":\s+(\d+)", block)
            vals.append(int(m.group(1)) if m else 0)
        out[name.group(1)] = tuple(vals)
    return (out, digest, per) if text else out


def objects(path):
    return sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]


def same_code(base, new):
    """0 if the objects of base and new (two directories, or two objects) hold the same kernels and the same device .text"""
    if os.path.isdir(base):
        bo, no = ({os.path.basename(o): o for o in objects(d)} for d in (base, new))
    else:
        bo, no = {os.path.basename(new): base}, {os.path.basename(new): new}
    bad = nobj = nker = 0
    for name in sorted(set(bo) | set(no)):
        if name not in bo or name not in no:
            print("unmatched object", name, "(only in %s)" % (new if name in no else base))
            bad += name in bo
            continue
        try:
            (kb, tb, pb), (kn, tn, pn) = kernels(bo[name], text=True), kernels(no[name], text=True)
        except subprocess.CalledProcessError:
            continue                                      # no device code in this object
        nobj += 1
        nker += len(kn)
        if set(kb) == set(kn):
            if tb != tn:
                print("differs", name, ".text", tb[:16], "->", tn[:16])
                bad += 1
            continue
        # other kernels in one build: those of both, one by one
        for k in sorted(set(kb) ^ set(kn)):
            print("only in", "NEW " if k in kn else "BASE", name, k)
        changed = [k for k in sorted(set(kb) & set(kn)) if k not in pb or k not in pn or pb[k] != pn[k]]
        for k in changed:
            print("differs", name, k)
        print("%s: %d kernels of both builds compared one by one, %d differ" % (name, len(set(kb) & set(kn)), len(changed)))
        bad += 1 if changed else 0
    print("%d objects with device code compared (%d kernels), %d differ or are unmatched" % (nobj, nker, bad))
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--same-code":
        return same_code(argv[1], argv[2])
    if argv and argv[0] == "--diff":
        base, new, strip = argv[1], argv[2], argv[3] if len(argv) > 3 else None
        worse = changed = total = 0
        for o in objects(new):
            b = os.path.join(base, os.path.basename(o))
            if not os.path.exists(b):
                continue
            try:
                kn, kb = kernels(o), kernels(b)
                if strip:
                    kn = {re.sub(strip, "", k): v for k, v in kn.items()}
                    kb = {re.sub(strip, "", k): v for k, v in kb.items()}
            except subprocess.CalledProcessError:
                continue                                  # no device code in this object
            for name, v in sorted(kn.items()):
                total += 1
                w = kb.get(name)
                if w is None:
                    print("unmatched", os.path.basename(o), name)
                    continue
                if w == v:
                    continue
                changed += 1
                bad = v[3] > w[3] or v[4] > w[4] or v[5] > w[5]
                worse += bad
                print("%s %s %s: vgpr/agpr/sgpr/vspill/sspill/scratch %s -> %s" % ("WORSE " if bad else "differs", os.path.basename(o), name, w, v))
        print("%d kernels compared, %d differ, %d gained a spill or scratch" % (total, changed, worse))
        return 1 if worse else 0
    for path in argv:
        for o in objects(path):
            try:
                for name, v in sorted(kernels(o).items()):
                    print(os.path.basename(o), name, *v)
            except subprocess.CalledProcessError:
                pass
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
