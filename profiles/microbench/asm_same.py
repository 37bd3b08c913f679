"""Are the kernels of two device assemblies (hipcc --offload-device-only -S) the same instructions?
    python profiles/microbench/asm_same.py parent/conv.s change/conv.s
Per kernel the lines between its label and its .Lfunc_end, with labels, comments and directives removed; prints the kernel
count and every kernel (demangled name kept mangled) whose instructions differ or that exists on one side only."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        s = line.split(';')[0].strip()
        m = re.match(r'^([A-Za-z_][\w$.]*):', s)
        if name is None:
            if m and not m.group(1).startswith('.L'):
                name, body = m.group(1), []
            continue
        if s.startswith('.Lfunc_end'):
            out[name], name = body, None
        elif s and not m and not s.startswith('.'):
            # (branch targets carry the function's ordinal in the file, .LBB<ordinal>_<block>: the ordinal is no instruction)
            body.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', s)))
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    only = sorted(set(ka) ^ set(kb))
    differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
    print('%s: %d functions, %s: %d functions; on one side only: %d; code differs in %d'
          % (a, len(ka), b, len(kb), len(only), len(differ)))
    print(''.join('   %s\n' % k for k in only + differ), end='')
    return 1 if only or differ else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
