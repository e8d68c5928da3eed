#!/usr/bin/env python
"""Print `symbol sha256` for every device function of libbdof's gfx950 ISA, sorted by symbol.

A host-code refactor must leave the device code alone.  The order in which hipcc emits template instantiations follows the host
code, so two builds are compared per symbol, not per file: run this on both trees and `diff` the outputs.  The hash covers the
function's instructions and its kernel descriptor (registers, LDS, scratch); the local labels, which carry the function's position
in the file (.LBB12_3, .Lfunc_end12), are renumbered out, and the assembler's trailing `; ...` comments are dropped: they
name such labels too, and the column they start in depends on how many digits the label's number had.

usage: python tools/isa_kernels.py [extra hipcc flags] > kernels.txt
"""
import hashlib
import re
import sys

from check_spills import KERNEL, device_isa

LOCAL = re.compile(r'(?:\.L|\b)(BB|func_begin|func_end|tmp|JTI)\d+')
DESC = re.compile(r'^\s*\.amdhsa_kernel\s+(\w+)')
COMMENT = re.compile(r'\s*;.*$')


def kernels(isa):
    """{symbol: text}: each function from its label to its .Lfunc_end, plus its .amdhsa_kernel block."""
    out, sym, desc = {}, None, None
    for line in isa.splitlines():
        m = KERNEL.match(line)
        if m:
            sym = m.group(1)
            out[sym] = []
        d = DESC.match(line)
        if d:
            desc = d.group(1)
        line = LOCAL.sub(lambda g: '.L' + g.group(1), COMMENT.sub('', line)).rstrip()
        if desc is not None:
            out.setdefault(desc, []).append(line)
            if line.strip() == '.end_amdhsa_kernel':
                desc = None
        elif sym is not None:
            out[sym].append(line)
            if line.startswith('.Lfunc_end'):
                sym = None
    return {k: '\n'.join(v) for k, v in out.items()}


def main():
    for sym, text in sorted(kernels(device_isa(sys.argv[1:] or None)).items()):
        print(sym, hashlib.sha256(text.encode()).hexdigest())


if __name__ == '__main__':
    main()
