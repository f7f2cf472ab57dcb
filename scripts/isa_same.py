"""Do two hipcc --save-temps ISA files (*-hip-amdgcn-amd-amdhsa-gfx950.s) hold the same code for the kernels they share?

Compares every function of the first file with the function of the same name in the second, instruction by instruction, after dropping
comments and renumbering basic-block labels (adding a kernel to a translation unit renumbers the labels of the ones after it).

    python scripts/isa_same.py before/post_kernels-hip-amdgcn-amd-amdhsa-gfx950.s after/post_kernels-hip-amdgcn-amd-amdhsa-gfx950.s
"""
from __future__ import annotations

import re
import sys


def functions(path: str) -> dict[str, list[str]]:
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\S+):[ \t]*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = []
        for line in m.group(2).splitlines():
            line = re.sub(r"\s*;.*$", "", line)
            line = re.sub(r"BB\d+_", "BB_", line)
            if line.strip():
                lines.append(line)
        out[m.group(1)] = lines
    return out


def main() -> int:
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    differ = 0
    for name, body in a.items():
        if name not in b:
            print(f"only in the first: {name}")
            differ += 1
            continue
        same = body == b[name]
        differ += not same
        print(f"{'identical' if same else 'DIFFERENT'} ({len(body)} lines)  {name}")
    for name in b.keys() - a.keys():
        print(f"only in the second: {name}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
