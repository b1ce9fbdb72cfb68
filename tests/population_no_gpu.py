"""What tests/test_minitaur_population.py and tests/test_kitchen_population.py share (a plain module: no tests, no fixtures): the population rows of the
malformed-argument table, the well-formed combinations, and where a source-text test finds a policy kernel's arguments."""
import ctypes as C
import os
import re

from conftest import REPO
from earl_benchmark_amd import _abi

CSRC = os.path.join(REPO, 'earl_benchmark_amd', 'csrc')


def pop_struct(n_policies=4, envs_per_policy=16, param_stride=4096):
  return _abi.PolicyPopulation(n_policies=n_policies, envs_per_policy=envs_per_policy, param_stride=param_stride)


def population_rows(count, n):
  """malformed populations for a policy of `count` parameters over n envs at env_offset 0 (check_population of csrc/policy_check.h, group 16, stride multiple 4)"""
  stride = (count + 3) // 4 * 4
  need = (n + 15) // 16
  return [pop_struct(0, 16, stride), pop_struct(-1, 16, stride), pop_struct(need, 8, stride), pop_struct(need, 0, stride), pop_struct(need, 24, stride),
          pop_struct(need, -16, stride), pop_struct(need, 16, count - 1), pop_struct(need, 16, stride + 1), pop_struct(need, 16, stride + 2),
          pop_struct(need, 16, 0), pop_struct(need - 1, 16, stride)]


def declared(name, n_args, after, before):
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'earl_physics.h')).read(), flags=re.S)
  m = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
  assert m, name + ' is not declared'
  assert len(m.group(1).split(',')) == len(_abi.SIGNATURES[name]) == n_args
  assert src.index(after) < m.start() < src.index(before)
  lib, host = _abi.load(), C.CDLL(_abi.HOST_LIB_PATH)
  assert hasattr(lib, name) and not hasattr(host, name)
  sig = _abi.SIGNATURES[name]
  assert sig[-2]._type_ is _abi.EpisodeSummary and any(getattr(a, '_type_', None) is _abi.PolicyPopulation for a in sig)


def summaries(p):
  return [None, _abi.EpisodeSummary(ret=p, success_last=p, first_success=p), _abi.EpisodeSummary(ret=p), _abi.EpisodeSummary(first_success=p)]


def policy_fields(env_header, struct, plain):
  """-> (the members of the plain struct, the closed-loop fields the policy struct obtains -- csrc/policy_closed_loop.h's ClosedLoopArgs<plain>, of which `struct`
  derives and to which it adds nothing --, the text of that header): where a source-text test looks for a policy kernel's arguments"""
  hdr = open(os.path.join(CSRC, env_header)).read()
  shared_hdr = open(os.path.join(CSRC, 'policy_closed_loop.h')).read()
  assert re.search(r'struct %s : ClosedLoopArgs<%s> \{\};' % (struct, plain), hdr), struct
  plain_body = re.search(r'struct %s \{(.*?)\n\};' % plain, hdr, flags=re.S).group(1)
  fields = re.search(r'struct ClosedLoopArgs : Plain \{(.*?)\n\};', shared_hdr, flags=re.S).group(1)
  return plain_body, fields, shared_hdr
