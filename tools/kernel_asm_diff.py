#!/usr/bin/env python3
"""Per-kernel instruction comparison of gfx950 .s files (hipcc -S
--cuda-device-only).  Every kernel of the OLD files is looked up by its
symbol in the NEW files; its instruction text is compared after dropping
comments, debug / location directives and the function's index in block
labels.  usage: kernel_asm_diff.py old.s[,old2.s] new.s[,new2.s] [filter]
Prints one line per kernel that differs or is missing, then a summary; exit
status 1 if any does."""
import re
import subprocess
import sys


def kernels(paths):
  out = {}
  for path in paths.split(','):
    text = open(path).read()
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    for m in re.finditer(r'^([A-Za-z_]\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text,
                         re.M | re.S):
      if m.group(1) not in names:
        continue
      body = []
      for line in m.group(2).split('\n'):
        line = line.split(';')[0].strip()
        if not line or re.match(r'\.(loc|file|cfi_|Ltmp|Lfunc_begin)', line):
          continue
        body.append(re.sub(r'\.LBB\d+_', '.LBB_', line))
      out[m.group(1)] = body
      names.discard(m.group(1))
    if names:
      sys.exit('%s: no body parsed for %d kernels' % (path, len(names)))
  return out


def main():
  old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
  filt = sys.argv[3] if len(sys.argv) > 3 else ''
  same = bad = 0
  for name, body in sorted(old.items()):
    dn = subprocess.run(['c++filt', name], capture_output=True,
                        text=True).stdout.strip()
    dn = dn.replace('(anonymous namespace)::', '')
    if filt not in dn:
      continue
    if name not in new:
      print('MISSING  %s' % dn[:110])
      bad += 1
    elif new[name] != body:
      print('DIFFERS  %5d -> %5d lines  %s' % (len(body), len(new[name]),
                                               dn[:100]))
      bad += 1
    else:
      same += 1
  extra = [n for n in new if n not in old]
  print('%d kernels identical, %d differ or are missing, %d only in new' %
        (same, bad, len(extra)))
  return 1 if bad else 0


if __name__ == '__main__':
  sys.exit(main())
