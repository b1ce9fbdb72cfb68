"""The compile-time tests' one way to a unit of csrc/ (a plain module: no tests, no fixtures): `unit(name)` cross-compiles csrc/<name> for gfx950 once per process,
with the flags of tools/scratch_in_loops.py and the compiler's resource remarks, and every reader of the assembly, the remarks and the recorded builds
(tests/golden/*.json) lives here.  No GPU is needed."""
import atexit
import functools
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import GOLDEN, REPO

HIPCC = '/opt/rocm/bin/hipcc'
CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')
FIGURES = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]')      # the order of profiles/policy_kernel_resources.txt
COMPILED = []                # every unit name handed to hipcc, in order: none twice (tests/test_kernel_build.py)
_LOCK = threading.Lock()     # guards COMPILED, _BUILT and _DIR
_BUILT = {}                  # unit name -> [its own lock, Unit | the tail of a failed compile's stderr | None]
_DIR = []


@functools.lru_cache(None)
def tool():
  """tools/scratch_in_loops.py as a module"""
  sys.path.insert(0, os.path.join(REPO, 'tools'))
  try:
    import scratch_in_loops
  finally:
    sys.path.pop(0)
  return scratch_in_loops


def need_hipcc():
  if shutil.which(HIPCC) is None:
    pytest.skip('needs hipcc (cross-compiles without a GPU)')


@functools.lru_cache(None)
def compiler_version():
  return subprocess.run([HIPCC, '--version'], capture_output=True, text=True).stdout


def recorded(filename, what='the parent build'):
  """tests/golden/<filename>, or a skip when this compiler is not the one it was recorded with"""
  want = json.load(open(os.path.join(GOLDEN, filename)))
  if want['compiler'] not in compiler_version():
    pytest.skip(what + ' was recorded with another compiler: ' + want['compiler'])
  return want


def recorded_figures():
  """{mangled kernel name: [the FIGURES tuple of every line on record]} from profiles/policy_kernel_resources.txt"""
  out = {}
  for line in open(os.path.join(REPO, 'profiles', 'policy_kernel_resources.txt')):
    if line.startswith('Name: '):
      parts = dict(p.split(': ') for p in line.strip().split(';'))
      out.setdefault(parts['Name'], []).append(tuple(int(parts[f]) for f in FIGURES))
  return out


def check_scratch_lines(lines, otherwise):
  """the scratch rule on lines of tool().report: a timestep loop holds no scratch instruction, and a line without one says one of the phrases of `otherwise`"""
  for ln in lines:
    print(ln)
    if 'timestep loop' in ln:
      assert ln.rstrip().endswith(': 0'), ln                             # scratch instructions inside the timestep loop
    else:
      assert any(phrase in ln for phrase in otherwise), ln


# ---------------------------------------------------------------------------------------------------------------- readers
def normalised_functions(lines):
  """{mangled name: the function's assembly lines} with comments, blank lines and the numbers of local labels removed"""
  out, i = {}, 0
  while i < len(lines):
    m = re.match(r'^(_Z\w+):\s', lines[i])
    if m:
      end = next(j for j in range(i, len(lines)) if lines[j].startswith('.Lfunc_end'))
      body = []
      for ln in lines[i + 1:end]:
        ln = ln.split(';')[0].rstrip()
        if ln.strip():
          body.append(re.sub(r'\.Ltmp\d+', '.Ltmp', re.sub(r'\.LBB\d+_', '.LBB_', ln)))
      out[m.group(1)] = body
      i = end
    i += 1
  return out


def digest(body):
  return hashlib.sha256('\n'.join(body).encode()).hexdigest()


def resources(remarks):
  """{demangled kernel name: dict(vgpr, agpr, scratch, occupancy, lds)} from -Rpass-analysis=kernel-resource-usage"""
  blocks = re.findall(r'Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?'
                      r'LDS Size \[bytes/block\]: (\d+)', remarks, flags=re.S)
  res = {}
  for mangled, vgpr, agpr, scratch, occ, lds in blocks:
    name = subprocess.run(['c++filt', mangled], capture_output=True, text=True).stdout.strip().replace('(anonymous namespace)::', '')
    res[re.sub(r'^void ', '', name).split('(')[0]] = dict(vgpr=int(vgpr), agpr=int(agpr), scratch=int(scratch), occupancy=int(occ), lds=int(lds))
  return res


def sgprs(asm):
  """{demangled kernel name: .sgpr_count} from the code-object metadata at the end of a unit's assembly"""
  out, name = {}, None
  for ln in asm:
    m = re.match(r'\s+(?:- )?\.(name|sgpr_count):\s+(\S+)', ln)
    if m and m.group(1) == 'name':
      name = m.group(2)
    elif m and name:
      full = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip().replace('(anonymous namespace)::', '')
      out[re.sub(r'^void ', '', full).split('(')[0]] = int(m.group(2))
  return out


class Unit:
  """one cross-compiled unit: `asm` (the assembly lines) and `remarks` (the compiler's stderr), and what the tests read out of them"""

  def __init__(self, name, asm, remarks):
    self.name, self.asm, self.remarks = name, asm, remarks

  @functools.cached_property
  def functions(self):
    return normalised_functions(self.asm)

  @functools.cached_property
  def digests(self):
    """{mangled name: [lines, sha256]}: the form of the recorded builds"""
    return {k: [len(b), digest(b)] for k, b in self.functions.items()}

  @functools.cached_property
  def nameless_digests(self):
    """`digests` with each function's own mangled name in its body (the .amdhsa_kernel and .section lines) replaced by a fixed token: comparable across a rename"""
    return {k: [len(b), digest([ln.replace(k, 'OWN_NAME') for ln in b])] for k, b in self.functions.items()}

  @functools.cached_property
  def resources(self):
    """{demangled kernel name: dict(vgpr, agpr, scratch, occupancy, lds, sgpr)}"""
    count = sgprs(self.asm)
    return {k: dict(v, sgpr=count[k]) for k, v in resources(self.remarks).items()}

  @functools.cached_property
  def figures(self):
    """{mangled name: the FIGURES tuple} of every function the remarks list"""
    return {blk.split()[0]: tuple(int(re.search(re.escape(f) + r': (\d+)', blk).group(1)) for f in FIGURES)
            for blk in self.remarks.split('remark: Function Name: ')[1:]}

  def scratch_report(self, kernels=None):
    return tool().report(self.name, self.asm, *(() if kernels is None else (kernels,)))


# ---------------------------------------------------------------------------------------------------------------- the cached cross-compile
def _compile(name):
  with _LOCK:
    if not _DIR:
      _DIR.append(tempfile.mkdtemp(prefix='kernel_build_'))
      atexit.register(shutil.rmtree, _DIR[0], ignore_errors=True)
    COMPILED.append(name)
  asm = os.path.join(_DIR[0], name + '.s')
  r = subprocess.run([HIPCC, *tool().FLAGS, '-Rpass-analysis=kernel-resource-usage', '-o', asm, os.path.join(CSRC, name)], capture_output=True, text=True, timeout=900)
  return Unit(name, open(asm).read().split('\n'), r.stderr) if r.returncode == 0 else r.stderr[-2000:]


def unit(name):
  """csrc/<name> cross-compiled with tool().FLAGS and the resource remarks: once per process, whoever asks and from whichever thread"""
  need_hipcc()
  with _LOCK:
    slot = _BUILT.setdefault(name, [threading.Lock(), None])
  with slot[0]:
    if slot[1] is None:
      slot[1] = _compile(name)
  assert isinstance(slot[1], Unit), slot[1]                              # (a failed compile is kept too: its dependants fail at once)
  return slot[1]


def units(names):
  """{name: unit(name)}; those not built yet compile side by side"""
  need_hipcc()
  names = list(names)
  with _LOCK:
    todo = [n for n in names if n not in _BUILT]
  if len(todo) > 1:
    with ThreadPoolExecutor(min(8, len(todo))) as pool:
      list(pool.map(unit, todo))
  return {n: unit(n) for n in names}
