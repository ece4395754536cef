"""The run-time switches of the package are the ones README.md documents, the retired ones are gone from the tree, and the shipped
library holds no diagnostic instantiation of the 1440-point spectrum kernels (no GPU: sources, README and the library's bytes)."""
import glob
import os
import re

from weatherbenchx_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'weatherbenchx_amd')

# decided in rounds 2-6 and folded to their shipped values (profiles/README.md, "Retired run-time switches")
RETIRED = (
    'WBX_ENS_ATOMS_TAPER', 'WBX_ENS_ATOMS_ROWS', 'WBX_ENS_ATOMS_NT', 'WBX_PATCH_ORDER', 'WBX_BINNED_ATOMS', 'WBX_BINNED_MERGED_MASK',
    'WBX_ATOMS_NT', 'WBX_BINNED_TARGET_WAVES', 'WBX_SPECTRUM_1440', 'WBX_SPECTRUM_LATFAST', 'WBX_SPECTRUM_1440_TEAMS',
    'WBX_SPECTRUM_ROUNDS', 'WBX_SPECTRUM_SKEW', 'WBX_SPECTRUM_LF_RUNS', 'WBX_SPECTRUM_LF_PRIO', 'WBX_SPECTRUM_PREFETCH',
    'WBX_SPECTRUM_ZL_EVEN', 'WBX_SPECTRUM_TILE_MB', 'WBX_SPECTRUM_DEBUG',
    'WBX_ALTERNATE_CHUNKS', 'WBX_FUSE_DET_SPECTRA', 'WBX_FOLD_DET_SPECTRA', 'WBX_FUSED_ACC_ADD', 'WBX_ENS_BINNED', 'WBX_ENS_TWIN_MASK',
    'WBX_DIRECT_RESULTS', 'WBX_ENS_PAIR_FORM', 'WBX_CHUNK_REPLAY', 'WBX_FLAT1_THREADS', 'WBX_FLAT1_MIN_ELEMENTS',
    'WBX_FLAT64_MIN_ELEMENTS', 'WBX_FLAT64_MIN_BLOCKS')


# (a retired name may be the head of a living one: WBX_FUSE_DET_SPECTRA_LATFAST)
_RETIRED_RE = r'(?<![A-Za-z0-9_])(' + '|'.join(RETIRED) + r')(?![A-Za-z0-9_])'


def _read(path):
  with open(path, encoding='utf-8', errors='replace') as f:
    return f.read()


def _variables_the_package_reads():
  names = set()
  for path in glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True):
    text = _read(path)
    reads = re.findall(r'\benviron\b\s*(?:\.\s*(?:get|pop|setdefault)\s*\(|\[)\s*([^,)\]]+)', text)
    reads += re.findall(r'\bos\.getenv\s*\(\s*([^,)]+)', text)
    for arg in reads:
      m = re.fullmatch(r'''['"]([A-Z0-9_]+)['"]''', arg.strip())
      assert m, f'{path}: an environment variable read through a name that is not a literal: {arg!r}'
      if m.group(1).startswith('WBX_'):
        names.add(m.group(1))
  for path in glob.glob(os.path.join(PKG, 'csrc', '*.hip')) + glob.glob(os.path.join(PKG, 'csrc', '*.hpp')):
    for arg in re.findall(r'\bgetenv\s*\(\s*([^)]*)\)', _read(path)):
      m = re.fullmatch(r'"(WBX_[A-Z0-9_]+)"', arg.strip())
      assert m, f'{path}: getenv of something else than a literal WBX_ name: {arg!r}'
      names.add(m.group(1))
  return names


def _readme_table():
  """{variable: who uses it} of README's environment table (rows `| \\`WBX_...\\` | default | what | who |`)."""
  rows = {}
  for line in _read(os.path.join(ROOT, 'README.md')).splitlines():
    if not line.startswith('| `WBX_'):
      continue
    cells = [c.strip() for c in line.strip().strip('|').split('|')]
    assert len(cells) == 4, f'README environment table: a row without four columns: {line}'
    for name in re.findall(r'`(WBX_[A-Z0-9_]+)`', cells[0]):
      assert name not in rows, f'{name} is listed twice'
      rows[name] = cells[3]
  return rows


def test_every_variable_the_package_reads_is_in_the_readme_table():
  table = _readme_table()
  documented = {name for name, who in table.items() if who.startswith('package')}
  assert _variables_the_package_reads() == documented
  assert not set(RETIRED) & set(table)


def test_retired_variables_are_gone_from_the_tree():
  assert len(set(RETIRED)) == 32
  pattern = re.compile(_RETIRED_RE)
  # outside profiles/ and the directories .gitignore keeps out of the repository (build products, caches, run outputs)
  ignored = [line.strip() for line in _read(os.path.join(ROOT, '.gitignore')).splitlines() if line.strip().endswith('/')]
  skipped_dirs = {'.git', 'profiles', 'build_diag'} | {line.rstrip('/').split('/')[-1] for line in ignored}
  hits = []
  for base, dirs, files in os.walk(ROOT):
    dirs[:] = [d for d in dirs if d not in skipped_dirs]
    for name in files:
      path = os.path.join(base, name)
      if name.endswith('.md') or path == os.path.abspath(__file__) or os.path.getsize(path) > 1 << 20:  # (no committed file is larger)
        continue
      hits += [f'{os.path.relpath(path, ROOT)}: {m}' for m in sorted(set(pattern.findall(_read(path))))]
  assert not hits, hits


def _library_bytes():
  assert os.path.exists(_hip.lib_path()), 'libwbx_hip.so is not built: run __graft_entry__.build()'
  with open(_hip.lib_path(), 'rb') as f:
    return f.read()


def _symbols_with(lib, needle):
  """The distinct runs of identifier characters in `lib` that contain `needle` (plain searches: the library is 17 MB)."""
  ident = re.compile(rb'[A-Za-z0-9_$.]*')
  found, at = set(), lib.find(needle)
  while at >= 0:
    start = at
    while start > 0 and (lib[start - 1:start].isalnum() or lib[start - 1:start] in (b'_', b'$', b'.')):
      start -= 1
    end = ident.match(lib, at).end()
    found.add(lib[start:end])
    at = lib.find(needle, end)
  return found


def test_shipped_library_holds_only_the_spectrum_kernels_it_can_launch():
  lib = _library_bytes()
  assert len(_symbols_with(lib, b'__device_stub__zspec1440_kernelI')) == 1
  assert len(_symbols_with(lib, b'__device_stub__zspec1440_latfast_kernelI')) == 1
  # (the RR = 0 instantiations at 256 threads went with the prefetch switch)
  assert len(_symbols_with(lib, b'__device_stub__zspec_fused_kernelI')) == 14
  assert not _symbols_with(lib, b'zspec1440_kernelILb1E'), 'the phase-stamped (PROF) instantiation is in the shipped library'
  knocked = [s for s in _symbols_with(lib, b'zspec1440_kernelILb0ELi') if re.search(rb'zspec1440_kernelILb0ELi[1-9]', s)]
  assert not knocked, f'knock-out (KNOCK) instantiations in the shipped library: {knocked}'
  named = [name for name in RETIRED if any(re.search(_RETIRED_RE.encode(), s) for s in _symbols_with(lib, name.encode()))]
  assert not named, f'the library still names retired variables: {named}'
