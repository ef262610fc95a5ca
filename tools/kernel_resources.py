"""Register / LDS / spill figures of every kernel in libcnmf_hip.so (read from the code object's metadata notes):
    python tools/kernel_resources.py [--isa] [--fp] [substring ...]
Unbundles the gfx950 code object from the shared library's .hip_fatbin section (clang-offload-bundler) and prints
`llvm-readelf --notes` per kernel: vgpr / agpr / sgpr counts, spills, LDS bytes, waves per SIMD the counts allow.
``--isa`` adds, per kernel, the number of instructions and two SHA-256 digests (12 hex digits each) of its disassembled
stream (`llvm-objdump -d --no-show-raw-insn --no-leading-addr`, addresses, labels and comments removed): the strict one
of the text as it stands, and one with every `0x...` literal masked (pc-relative and kernel-argument offsets move when
code elsewhere in the library does).  Two builds of one kernel with equal digests run the same instructions; diff the
two tables.  ``--fp`` prints instead, per kernel, the histogram of its floating-point opcodes (``v_*_f64*``, ``v_*_f32*``):
two builds of a kernel whose v_fma / v_mul / v_add split differs contract their arithmetic differently and will not give
the same bits.  CNMF_LIB_PATH names another build of the library."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_streams(co):
    """{demangled kernel name: [instruction, ...]} of a code object (addresses, labels and comments removed)"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          check=True, capture_output=True, text=True).stdout
    text = subprocess.run(["c++filt"], input=text, capture_output=True, text=True).stdout
    out, lines = {}, None
    for line in text.splitlines():
        head = re.match(r"^[0-9a-fA-F]* ?<(.*)>:\s*$", line)
        if head:
            if not head.group(1).startswith("L"):          # a symbol opens a function; local labels (<L12>:) are dropped
                lines = out.setdefault(head.group(1), [])
            continue
        ins = re.sub(r"\s+", " ", re.sub(r"(//|;).*$", "", line)).strip()
        ins = re.sub(r"\s*<[^>]*>", "", ins)                # branch targets named after labels
        if ins and lines is not None:
            lines.append(ins)
    return out


def isa_digests(co):
    """{demangled kernel name: (instructions, strict digest, masked digest)} of a code object"""
    out = {}
    for name, lines in kernel_streams(co).items():
        body = "\n".join(lines).encode()
        masked = re.sub(r"0x[0-9a-fA-F]+", "0x#", "\n".join(lines)).encode()
        out[name] = (len(lines), hashlib.sha256(body).hexdigest()[:12], hashlib.sha256(masked).hexdigest()[:12])
    return out


def fp_histograms(co):
    """{demangled kernel name: "opcode=count ..." over its v_*_f64* / v_*_f32* instructions, sorted by opcode}"""
    out = {}
    for name, lines in kernel_streams(co).items():
        hist = {}
        for ins in lines:
            op = ins.split(" ", 1)[0]
            if re.match(r"^v_\w+_f(64|32)", op):
                hist[op] = hist.get(op, 0) + 1
        out[name] = " ".join("%s=%d" % kv for kv in sorted(hist.items())) or "-"
    return out


def main():
    so = os.environ.get("CNMF_LIB_PATH", os.path.join(ROOT, "cnmf_amd", "libcnmf_hip.so"))
    isa, fp = "--isa" in sys.argv[1:], "--fp" in sys.argv[1:]
    pats = [a for a in sys.argv[1:] if a not in ("--isa", "--fp")]
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        co = os.path.join(tmp, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        names = subprocess.run(["c++filt"], input=notes, capture_output=True, text=True).stdout
        if fp:
            for name, hist in sorted(fp_histograms(co).items()):
                if not pats or any(p in name for p in pats):
                    print("%s | %s" % (name[:150], hist))
            return
        digests = isa_digests(co) if isa else {}
    rows = []
    for blk in re.split(r"\n\s+- \.agpr_count:", names)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: (re.search(r"\.%s:\s+(\S+)" % key, blk) or [None, "?"])[1]
        name = re.search(r"\.name:\s+(.*)", blk)
        name = name.group(1).strip().strip("'") if name else "?"
        if pats and not any(p in name for p in pats):
            continue
        v, a = get("vgpr_count"), get("agpr_count")
        tot = (int(v) if v.isdigit() else 0)
        waves = min(8, 512 // max(8, (tot + 7) // 8 * 8)) if tot else 0
        rows.append((name, v, a, get("sgpr_count"), get("vgpr_spill_count"), get("sgpr_spill_count"),
                     get("group_segment_fixed_size"), get("private_segment_fixed_size"), waves))
    extra = "%-6s %-12s %-12s " % ("insns", "strict", "masked") if isa else ""
    print("%-6s %-5s %-5s %-7s %-7s %-8s %-8s %-5s %s%s" % ("vgpr", "agpr", "sgpr", "vspill", "sspill", "lds", "scratch", "waves", extra, "kernel"))
    for r in sorted(rows):
        extra = "%-6s %-12s %-12s " % digests.get(r[0], ("?", "?", "?")) if isa else ""
        print("%-6s %-5s %-5s %-7s %-7s %-8s %-8s %-5s %s%s" % (r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], extra, r[0][:150]))


if __name__ == "__main__":
    main()
