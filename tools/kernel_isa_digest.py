#!/usr/bin/env python3
"""One line per device symbol of a translation unit: instruction count, digest of the instruction text, digest of the kernel
descriptor (device-only compile with build.sh's code-generation flags, no GPU needed).  Addresses and raw bytes are stripped, so two
trees whose outputs `diff` equal compile to the same instructions.
usage: tools/kernel_isa_digest.py [file.hip ...]    (default: the translation units of build.sh's TUS line)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tus = sys.argv[1:] or [f"scldm_amd/csrc/{t}.hip" for t in re.search(r'^TUS="([^"]*)"', open(os.path.join(root, "build.sh")).read(), re.M)[1].split()]
flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-I", "include", *os.environ.get("SCLDM_HIPCC_FLAGS", "").split()]
digest = lambda b: hashlib.sha256(b).hexdigest()[:16]


def run(*cmd):
    return subprocess.run(cmd, cwd=root, check=True, capture_output=True, text=True).stdout


for tu in tus:
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "device.co")
        run("hipcc", *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", tu, "-o", co)
        # kernel descriptors: the 64-byte `<kernel>.kd` objects of .rodata, read straight from the file
        elf = run("llvm-readelf", "-S", "-s", "-C", "-W", co)
        sec = {m[1]: (int(m[2], 16), int(m[3], 16)) for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)", elf, re.M)}
        addr, off = sec[".rodata"]
        blob = open(co, "rb").read()
        kd = {}
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+OBJECT\s+\S+\s+\S+\s+\d+\s+(.+) \(\.kd\)$", elf, re.M):
            at = int(m[1], 16) - addr + off
            kd[m[3]] = digest(blob[at:at + int(m[2])])
        # instruction text per symbol of .text, without the `// address: bytes <target>` comment
        syms, cur = {}, None
        for line in run("llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
            if m:
                cur = syms.setdefault(m[1], [])
            elif cur is not None and line.startswith("\t"):
                cur.append(" ".join(line.split("//")[0].split()))
        # a symbol ends at its last s_endpgm: what follows is the padding of its section (s_code_end / s_nop / elided zeros), which
        # depends on where the linker put the symbol (last of .text, or a template instantiation in a section of its own)
        for body in syms.values():
            ends = [i for i, ins in enumerate(body) if ins.startswith("s_endpgm")]
            if ends:
                del body[ends[-1] + 1:]
    print(f"# {tu}: {len(syms)} symbols, {sum(map(len, syms.values()))} instructions")
    for name in sorted(syms):
        print(f"{tu} | {name} | {len(syms[name])} insts | isa {digest(chr(10).join(syms[name]).encode())} | kd {kd.get(name, '-')}")
