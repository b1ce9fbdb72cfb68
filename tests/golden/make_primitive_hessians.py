#!/usr/bin/env python3
"""Record Hessians and right-hand sides that real timesteps of this project's own CPU statement of the stepper (oracle/physics_oracle.py) hand to its linear solver, as
the fixture tests/golden/primitive_hessians.npz of tests/test_physics_primitives_gpu.py: the door (nv 10) and the peg (nv 15), both reset at the goal (hand on the handle,
peg in the hole: contact rows in the Hessian) and driven by random actions.  Every (H, g) passed to numpy.linalg.solve with H of the model's size is a candidate -- the
active-set iterations' M + J' D J and the integration's M + dt B -- and an even subsample is kept.  Numbers only; the tests read the file, never oracle/.

Usage:  python tests/golden/make_primitive_hessians.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
KEEP, STEPS = 160, 24


def record(make_env, nv, adim, seed):
  seen = []
  real = np.linalg.solve

  def spy(a, b):
    if getattr(a, 'shape', None) == (nv, nv) and np.ndim(b) == 1:
      seen.append((np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)))
    return real(a, b)
  np.linalg.solve = spy
  try:
    env = make_env()
    env.reset()
    rng = np.random.default_rng(seed)
    for _ in range(STEPS):
      env.step(rng.uniform(-1, 1, adim))
  finally:
    np.linalg.solve = real
  pick = np.linspace(0, len(seen) - 1, KEEP).round().astype(int)
  H = np.stack([seen[i][0] for i in pick])
  H = 0.5 * (H + H.transpose(0, 2, 1))
  return H, np.stack([seen[i][1] for i in pick]), len(seen)


def main():
  from oracle import physics_oracle as po
  from oracle.sawyer_oracle import SawyerDoorOracle, SawyerPegOracle
  models = os.path.join(REPO, 'earl_benchmark_amd', 'models')
  out = {}
  for name, cls, nv in (('door', SawyerDoorOracle, 10), ('peg', SawyerPegOracle, 15)):
    lm = po.LinkModel(os.path.join(models, f'sawyer_{name}_links.npz'))
    H, g, total = record(lambda: cls(lm, reset_at_goal=True, seed=5), nv, 4, seed=nv)
    print(name, 'solves seen', total, 'kept', len(H), 'condition of the equilibrated H: max %.3g' % max(np.linalg.cond(h / np.sqrt(np.outer(np.diag(h), np.diag(h)))) for h in H))
    out[f'{name}_H'], out[f'{name}_g'] = H, g
  np.savez_compressed(os.path.join(HERE, 'primitive_hessians.npz'), **out)


if __name__ == '__main__':
  main()
