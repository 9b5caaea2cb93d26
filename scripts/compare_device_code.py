#!/usr/bin/env python
"""Compares the gfx950 device code of two builds of libspeecht_hip.so kernel by kernel, without a GPU.

  python scripts/compare_device_code.py OLD.so NEW.so [--out FILE.json]

Every code object bundled in the libraries' .hip_fatbin section is taken out (clang offload bundles, uncompressed), its function
symbols are read with llvm-readelf, and each kernel's machine code bytes are hashed.  Reported: kernels only in one library, and
kernels in both whose bytes differ.  Used to state that a change left the existing kernels' code as it was."""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
LLVM_BIN = os.environ.get('LLVM_BIN', os.path.join(os.path.dirname(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), '..', 'llvm', 'bin'))


def code_objects(path):
  """The gfx950 ELF images in a library, in file order."""
  data = open(path, 'rb').read()
  at = data.find(MAGIC)
  if at < 0:
    raise SystemExit('{}: no uncompressed offload bundle found'.format(path))
  images = []
  while at >= 0:
    count, = struct.unpack_from('<Q', data, at + len(MAGIC))
    pos = at + len(MAGIC) + 8
    for _ in range(count):
      offset, size, triple_len = struct.unpack_from('<QQQ', data, pos)
      triple = data[pos + 24:pos + 24 + triple_len].decode()
      pos += 24 + triple_len
      if 'gfx950' in triple and size:
        images.append(data[at + offset:at + offset + size])
    at = data.find(MAGIC, pos)
  return images


def kernels(image):
  """{symbol: sha256 of its bytes} for the functions of one code object."""
  with tempfile.NamedTemporaryFile(suffix='.co') as f:
    f.write(image)
    f.flush()
    sections = subprocess.check_output([os.path.join(LLVM_BIN, 'llvm-readelf'), '-S', '-W', f.name], text=True)
    symbols = subprocess.check_output([os.path.join(LLVM_BIN, 'llvm-readelf'), '-s', '-W', f.name], text=True)
  m = re.search(r'\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', sections)
  if not m:
    return {}
  addr, offset = int(m.group(1), 16), int(m.group(2), 16)
  out = {}
  for line in symbols.splitlines():
    parts = line.split()
    if len(parts) >= 8 and parts[3] == 'FUNC' and parts[6] != 'UND':
      value, size, name = int(parts[1], 16), int(parts[2]), parts[7]
      out[name] = hashlib.sha256(image[offset + value - addr:offset + value - addr + size]).hexdigest()
  return out


def library(path):
  table = {}
  for image in code_objects(path):
    for name, digest in kernels(image).items():
      table.setdefault(name, []).append(digest)
  return table


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('old')
  parser.add_argument('new')
  parser.add_argument('--out')
  args = parser.parse_args()
  old, new = library(args.old), library(args.new)
  result = dict(functions_old=len(old), functions_new=len(new), only_old=sorted(set(old) - set(new)), only_new=sorted(set(new) - set(old)),
                differ=sorted(n for n in set(old) & set(new) if sorted(old[n]) != sorted(new[n])))
  result['identical'] = len(set(old) & set(new)) - len(result['differ'])
  text = json.dumps(result, indent=1, sort_keys=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')
  print(text)
  return 0


if __name__ == '__main__':
  sys.exit(main())
