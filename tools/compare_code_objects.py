"""The gfx950 code objects of two builds of weatherbenchx_amd/csrc, unit by unit and kernel by kernel (a compile-side check:
no GPU).  For every object file of both build directories: the .hip_fatbin section (llvm-objcopy), its gfx950 member
(clang-offload-bundler), the disassembly (llvm-objdump -d) cut into functions, and the kernels' resource metadata
(llvm-readelf --notes: VGPRs, SGPRs, scratch, LDS).  Prints one table: per unit, whether the code objects are byte-identical;
otherwise which kernels left, which are new, and for every kernel of both builds whether its instruction sequence and resources
are the same.  The one difference tolerated -- and counted -- is the literal of an s_add_u32 / s_addc_u32 directly behind an
s_getpc_b64: a pc-relative address, which moves when other kernels leave the object.
usage: python tools/compare_code_objects.py <old>/weatherbenchx_amd/csrc/build <new>/weatherbenchx_amd/csrc/build
exit status 1 when a kernel that both builds have differs in anything else."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
RESOURCES = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def tool(name, *args):
  return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
  """The gfx950 code object inside `obj`, or None for a unit without device code."""
  fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'co')
  for f in (fat, co):
    if os.path.exists(f):
      os.remove(f)
  try:
    tool('llvm-objcopy', '--dump-section', '.hip_fatbin=' + fat, obj, os.path.join(tmp, 'stripped'))
  except subprocess.CalledProcessError as e:
    if 'not found' in e.stderr:  # a unit of host code only has no such section
      return None
    raise
  if not os.path.exists(fat) or os.path.getsize(fat) == 0:
    return None
  tool('clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fat, '--targets=' + TARGET, '--output=' + co)
  return co if os.path.getsize(co) else None


def functions(co):
  """{symbol: [instruction, ...]} of the disassembly (the address / encoding comments dropped)."""
  out, cur = {}, None
  for line in tool('llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
    m = re.match(r'^<(.+)>:$', line)
    if m:
      cur = out.setdefault(m.group(1), [])
    elif cur is not None and line.startswith('\t'):
      cur.append(line.split('//')[0].strip())
  return out


def resources(co):
  """{kernel symbol: (vgprs, sgprs, scratch bytes, LDS bytes)} from the amdhsa.kernels note."""
  out = {}
  for entry in re.split(r'\n\s*- \.agpr_count:', tool('llvm-readelf', '--notes', co))[1:]:
    name = re.search(r'^    \.name:\s*(\S+)', entry, re.M).group(1)  # (four spaces: the kernel's own keys, not an argument's)
    out[name] = tuple(int(re.search(r'^    ' + re.escape(k) + r':\s*(\d+)', entry, re.M).group(1)) for k in RESOURCES)
  return out


def same_but_pc_literals(a, b):
  """(equal?, number of pc-relative literals that differ) of two instruction lists."""
  if len(a) != len(b):
    return False, 0
  moved = 0
  for i, (x, y) in enumerate(zip(a, b)):
    if x == y:
      continue
    behind_getpc = any(a[j].startswith('s_getpc_b64') for j in (i - 1, i - 2) if j >= 0)
    xs, ys = x.rsplit(',', 1), y.rsplit(',', 1)
    if behind_getpc and x.startswith(('s_add_u32', 's_addc_u32')) and xs[0] == ys[0]:
      moved += 1
      continue
    return False, moved
  return True, moved


def main(old_dir, new_dir):
  units = sorted({os.path.basename(f) for d in (old_dir, new_dir) for f in glob.glob(os.path.join(d, '*.o'))})
  bad = 0
  print(f'old: {old_dir}\nnew: {new_dir}\n')
  print(f'{"unit":24s} {"old bytes":>10s} {"new bytes":>10s} {"kernels":>9s}  verdict')
  details = []
  with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
    for u in units:
      a, b = os.path.join(old_dir, u), os.path.join(new_dir, u)
      if not (os.path.exists(a) and os.path.exists(b)):
        print(f'{u:24s} only in the {"old" if os.path.exists(a) else "new"} build')
        bad += 1
        continue
      ca, cb = code_object(a, ta), code_object(b, tb)
      if ca is None or cb is None:
        print(f'{u:24s} {"-":>10s} {"-":>10s} {"-":>9s}  {"no device code" if ca is None and cb is None else "DEVICE CODE IN ONE BUILD ONLY"}')
        bad += (ca is None) != (cb is None)
        continue
      da, db = open(ca, 'rb').read(), open(cb, 'rb').read()
      ra, rb = resources(ca), resources(cb)
      if da == db:
        print(f'{u:24s} {len(da):10d} {len(db):10d} {len(ra):4d}/{len(rb):<4d}  byte-identical (sha256 {hashlib.sha256(da).hexdigest()[:12]})')
        continue
      fa, fb = functions(ca), functions(cb)
      gone, new = sorted(set(ra) - set(rb)), sorted(set(rb) - set(ra))
      same = moved_kernels = differ = res_differ = 0
      lines = []
      for k in sorted(set(ra) & set(rb)):
        eq, moved = same_but_pc_literals(fa[k], fb[k])
        if ra[k] != rb[k]:
          res_differ += 1
          lines.append(f'  RESOURCES DIFFER {k}: {ra[k]} -> {rb[k]}')
        if not eq:
          differ += 1
          lines.append(f'  INSTRUCTIONS DIFFER {k}: {len(fa[k])} -> {len(fb[k])} instructions')
        elif moved:
          moved_kernels += 1
          lines.append(f'  same but {moved} pc-relative literal(s): {k}')
        else:
          same += 1
      bad += differ + res_differ
      print(f'{u:24s} {len(da):10d} {len(db):10d} {len(ra):4d}/{len(rb):<4d}  {len(gone)} kernels gone, {len(new)} new; of the '
            f'{len(set(ra) & set(rb))} in both: {same} identical, {moved_kernels} identical but for pc-relative literals, '
            f'{differ} different; resources (VGPRs, SGPRs, scratch, LDS) {"equal" if not res_differ else f"DIFFER in {res_differ}"}')
      details.append((u, [f'  gone: {k}' for k in gone] + [f'  NEW: {k}' for k in new] + lines))
      bad += len(new)
  for u, lines in details:
    print(f'\n{u}:')
    print('\n'.join(lines))
  print(f'\n{"OK" if not bad else "FAILED"}: {bad} unexpected difference(s)')
  return 1 if bad else 0


if __name__ == '__main__':
  if len(sys.argv) != 3:
    sys.exit(__doc__)
  sys.exit(main(sys.argv[1], sys.argv[2]))
