"""Developer tool (no GPU): registers, scratch and spills of the built kernels whose name contains one of the given substrings.
usage: python scripts/kernel_regs.py place_hash64 place_packed16s [--lib=path.so] [--isa]
--isa: per kernel also the instruction count and a SHA-1 of its disassembly text, for telling whether a source change moved the
code of a kernel at all.  What depends on where the kernel lies in the code object is taken out of the text first: addresses and
encodings, branch offsets and their symbol-relative labels, and the literal of a pc-relative address (the add behind s_getpc_b64)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rappas_amd.tools import check_isa as ci


def kernel_text(co):
    """{symbol: [instruction text, ...]} of a code object, position-dependent parts removed"""
    dis = subprocess.run([ci._tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    out, cur, after_getpc = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
        if not ins:
            continue
        if re.match(r"s_(c?branch|call)\S* ", ins):
            ins = ins.split(" ")[0] + " <target>"
        if after_getpc and re.match(r"s_addc?_u32 ", ins):  # the two halves of symbol - pc
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<rel>", ins)
        after_getpc = 3 if ins.startswith("s_getpc_b64") else max(0, after_getpc - 1)
        cur.append(ins)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    isa = "--isa" in sys.argv[1:]
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rappas_amd", "librappas_place.so")
    for a in sys.argv[1:]:
        if a.startswith("--lib="):
            lib = a[6:]
    with tempfile.TemporaryDirectory() as d:
        for co in ci.device_code_objects(lib, d):
            notes = subprocess.run([ci._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            text = kernel_text(co) if isa else {}
            for e in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
                n = re.search(r"\.name:\s+(\S+)", e)
                if not n or not any(s in n.group(1) for s in args):
                    continue
                name = subprocess.run(["c++filt", n.group(1)], capture_output=True, text=True).stdout.strip()
                g = lambda k: re.search(r"\." + k + r":\s+(\d+)", e).group(1)
                row = f"{name[:110]:110s} vgpr {g('vgpr_count'):>3s} sgpr {g('sgpr_count'):>3s} scratch {g('private_segment_fixed_size'):>4s} B  spills {g('vgpr_spill_count')}"
                if isa:
                    ins = text.get(n.group(1), [])
                    row += f"  insts {len(ins):>6d}  sha1 {hashlib.sha1(chr(10).join(ins).encode()).hexdigest()[:16]}"
                print(row)


if __name__ == "__main__":
    main()
