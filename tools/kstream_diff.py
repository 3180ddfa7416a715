"""Did a change move the existing kernels? Compare the gfx950 instruction streams of two libaquad.so builds.

  python tools/kstream_diff.py PARENT.so NEW.so [--appended Lb0E ...]

Takes the gfx950 code object out of each library's fat binary, disassembles it (llvm-objdump -d), strips
the addresses and the pc-relative displacement of globals (s_getpc_b64 + s_add_u32 / s_addc_u32 literals,
which move with code placement), and compares every kernel of PARENT with its twin in NEW. --appended
names the mangled template arguments a change appended to k_stream's list with a default (one defaulted
bool: Lb0E), so that PARENT's k_stream<...> finds NEW's k_stream<..., false>. Then prints, from NEW's code
object metadata, VGPRs / SGPRs / scratch / LDS / workgroup size of the kernels PARENT does not have (`new:`
lines, kernels of any name). Exit status 1 if any instruction stream differs or NEW holds a kernel that
PARENT lacks: a change that means to add none passes only when the two sets are equal in both directions.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
KSTREAM_TAIL = "EEvNS_12StreamParamsE"


def code_object(so, work, tag):
    fat = os.path.join(work, tag + ".fatbin")
    co = os.path.join(work, tag + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    return co


def streams(co):
    """symbol -> instructions, addresses stripped."""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True,
                          text=True, check=True).stdout
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ln = re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", ln).strip()
        if cur is None or not ln:
            continue
        if cur and cur[-1].startswith("s_getpc_b64") and ln.startswith("s_add_u32"):
            ln = re.sub(r"0x[0-9a-f]+$", "PCREL_LO", ln)
        if len(cur) > 1 and cur[-2].startswith("s_getpc_b64") and ln.startswith("s_addc_u32"):
            ln = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "PCREL_HI", ln)
        cur.append(ln)
    return out


def demangle(name):
    r = subprocess.run(["c++filt", name], capture_output=True, text=True)
    return r.stdout.strip() or name


def metadata(co):
    """kernel symbol -> {field: int} from the code object's notes."""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True,
                           check=True).stdout
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        nm = re.search(r"\.name:\s*(\S+)", blk)
        if nm:
            out[nm.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s*(\d+)\s*$", blk, flags=re.M)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--appended", default="Lb0E", help="mangled defaulted template arguments appended to k_stream")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        cp, cn = code_object(a.parent, work, "parent"), code_object(a.new, work, "new")
        P, N = streams(cp), streams(cn)
        meta = metadata(cn)
    same = {True: 0, False: 0}
    other = {True: 0, False: 0}
    twins = set()
    for name, ins in sorted(P.items()):
        ks = "k_stream" in name
        twin = name.replace("E" + KSTREAM_TAIL, "E" + a.appended + KSTREAM_TAIL) if ks and name not in N else name
        twins.add(twin)
        ok = N.get(twin) == ins
        (same if ks else other)[ok] += 1
        if not ok:
            new = N.get(twin)
            where = "missing" if new is None else next((i for i, (x, y) in enumerate(zip(ins, new)) if x != y), min(len(ins), len(new)))
            print("DIFFERS", demangle(name), where if new is None else (where, ins[where:where + 1], new[where:where + 1]))
    print("k_stream instances identical: %d different: %d" % (same[True], same[False]))
    print("other kernels identical: %d different: %d" % (other[True], other[False]))
    added = sorted(n for n in N if n not in twins)   # kernels of NEW without a twin in PARENT, of any name
    for name in added:
        m = meta.get(name, {})
        print("new:", demangle(name), "vgpr", m.get("vgpr_count"), "sgpr", m.get("sgpr_count"), "scratch",
              m.get("private_segment_fixed_size"), "lds", m.get("group_segment_fixed_size"), "workgroup",
              m.get("max_flat_workgroup_size"))
    sys.exit(1 if same[False] or other[False] or added else 0)


if __name__ == "__main__":
    main()
