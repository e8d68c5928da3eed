#!/usr/bin/env python
"""Print `symbol sha256 sha256(descriptor) sha256(opcodes)` for every device function of libbdof's gfx950 ISA, sorted by symbol.

A host-code refactor must leave the device code alone.  The order in which hipcc emits template instantiations follows the host
code, so two builds are compared per symbol, not per file: run this on both trees and `diff` the outputs.  The hash covers the
function's instructions and its kernel descriptor (registers, LDS, scratch); the local labels, which carry the function's position
in the file (.LBB12_3, .Lfunc_end12), are renumbered out, and the assembler's trailing `; ...` comments are dropped: they
name such labels too, and the column they start in depends on how many digits the label's number had.

A device-side refactor (a helper factored out of several kernels) keeps the instructions and the resources but not their order
or the register names, so the first hash moves.  Two further columns say what did not: the hash of the `.amdhsa_kernel` block
alone (registers, LDS, scratch, hence occupancy), and the hash of the function's sorted opcode column — the instruction
mnemonics without operands, labels and directives, i.e. the histogram of what the function executes.

usage: python tools/isa_kernels.py [extra hipcc flags] > kernels.txt
"""
import hashlib
import re
import sys

from check_spills import KERNEL, device_isa

LOCAL = re.compile(r'(?:\.L|\b)(BB|func_begin|func_end|tmp|JTI)\d+')
DESC = re.compile(r'^\s*\.amdhsa_kernel\s+(\w+)')
COMMENT = re.compile(r'\s*;.*$')
LABEL = re.compile(r'^[.\w$]+:')


def kernel_parts(isa):
    """{symbol: (body lines, descriptor lines)}: each function from its label to its .Lfunc_end, and its .amdhsa_kernel block."""
    out, sym, desc = {}, None, None
    for line in isa.splitlines():
        m = KERNEL.match(line)
        if m:
            sym = m.group(1)
            out[sym] = ([], [])
        d = DESC.match(line)
        if d:
            desc = d.group(1)
        line = LOCAL.sub(lambda g: '.L' + g.group(1), COMMENT.sub('', line)).rstrip()
        if desc is not None:
            out.setdefault(desc, ([], []))[1].append(line)
            if line.strip() == '.end_amdhsa_kernel':
                desc = None
        elif sym is not None:
            out[sym][0].append(line)
            if line.startswith('.Lfunc_end'):
                sym = None
    return out


def kernels(isa):
    """{symbol: text}: the function's body followed by its descriptor."""
    return {k: '\n'.join(body + desc) for k, (body, desc) in kernel_parts(isa).items()}


def opcodes(body):
    """The sorted opcode column of a function's body: the first word of every line that is neither a label nor a directive."""
    ops = []
    for line in body:
        t = line.strip()
        if t and not t.startswith('.') and not LABEL.match(t):
            ops.append(t.split()[0])
    return sorted(ops)


def sha(lines):
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def table(isa):
    """[(symbol, full hash, descriptor hash, opcode hash)], sorted by symbol."""
    return [(sym, sha(body + desc), sha(desc), sha(opcodes(body))) for sym, (body, desc) in sorted(kernel_parts(isa).items())]


def main():
    for row in table(device_isa(sys.argv[1:] or None)):
        print(*row)


if __name__ == '__main__':
    main()
