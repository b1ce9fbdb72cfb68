"""Captured closed-loop stepping of the physics envs (door, peg, kitchen, minitaur): the counterpart of tabletop's `StepGraph` (envs/tabletop.py).

Each captured step is the env's own T = 1 fused rollout launch, through the `_clocked` entry points of include/earl_physics.h: every random draw a
step makes is keyed by a counter the host passes BY VALUE in the cfg struct (the door / peg / minitaur goal-switch draws: `step_counter`, the kitchen's
sensor noise: `counter`), and a capture would freeze that value.  So the captured launch of step t passes the OFFSET t, and the kernel adds a base it
reads from a device word when it runs (`clock[0]` for `counter`, `clock[1]` for `step_counter`); replay() writes both words from the env's host
counters before every replay.  A replay is then bit-identical to T eager step() calls.

The env's side is ONE set of hooks on `PhysicsEnv` (envs/physics_env.py): `_graph_check`, `_new_graph_out`, `_graph_capture`, `_graph_clock`, `_graph_advance` and
`_graph_bounds` are the base's (the cfg field a capture restores and the bounds are the subclass's class data); `_graph_step` and `_graph_info` are the subclass's.
"""
import torch


class PhysicsStepGraph:
  """T gym-style `step()` launches of one physics env batch captured once into a HIP graph and replayed with a single host call.

    g = env.make_step_graph(T)                  # action ring: the caller (or its own captured kernels) fills g.actions[t] ([T, N, A]) before replay
    g = env.make_step_graph(T, policy=pi)       # pi(obs [N, D]) -> actions [N, A] is captured INTO the graph between the steps: step t
                                                #   consumes pi(observation of step t - 1); `g.obs_in` holds the observation the first
                                                #   step of a replay starts from and is refreshed by the graph's last node
    obs, reward, done, info = g.replay()        # [T, N, ...] tensors: the outputs of the T steps

  A = 4 (door, peg), 9 (kitchen), 8 (minitaur).  The graph is one straight chain on one stream.  `info` holds what the launches write: the keys of the
  env's batched step() info dict -- door / peg: 'is_successful', 'status' and, with info='full', the reference's seven evaluate_state entries (the door's
  earl_sawyer_door_info launch is part of the graph); minitaur: 'success', 'status'; kitchen: 'success', 'is_successful', 'status' -- NOT the kitchen's full
  env_info (its noisy velocity readings are drawn by a separate launch on the host's counter), which eager step() with info='full' returns.
  Lifelong goal switching (cfg.goal_change_frequency, as set when the graph is built) runs inside the graph for door, peg and minitaur, where the switch is
  in the kernel; the kitchen switches goals on the host, so its graph refuses it.  The minitaur's out-of-bounds action check cannot raise inside a graph:
  each step records a device flag (g.action_out_of_bounds [T]) and g.check_actions() synchronises and raises the reference's ValueError."""

  def __init__(self, env, T, policy=None):
    u = env.unwrapped if hasattr(env, 'unwrapped') else env
    if u.scalar_api:
      raise ValueError('make_step_graph is for the batched API (scalar_api=False)')
    if u.device.type != 'cuda':
      raise ValueError('make_step_graph captures HIP launches: device="cuda" only')
    if int(T) < 1:
      raise ValueError(f'make_step_graph needs T >= 1, got {T}')
    u._graph_check()
    self.env, self.T, self.policy = u, int(T), policy
    n, dev, A = u.num_envs, u.device, u.action_space.shape[0]
    with torch.cuda.device(dev):
      self.actions = torch.zeros(self.T, n, A, dtype=torch.float32, device=dev)
      self.out = u._new_graph_out(self.T)
      self.obs, self.reward, self.done, self.success, self.status = (self.out[k] for k in ('obs', 'reward', 'done', 'success', 'status'))
      self.obs_in = u.last_obs.clone()                         # the observation the env returned last (written by reset and by every step)
      self.clock = torch.zeros(2, dtype=torch.int64, device=dev)      # the two uint64 clock words (two's complement) the captured launches read
      self.action_out_of_bounds = torch.zeros(self.T, dtype=torch.bool, device=dev)
      self._oob = torch.zeros(self.T, A, dtype=torch.bool, device=dev) if u._graph_bounds is not None else None
      if policy is not None:                                   # warm the policy up outside the capture (lazy library initialisation)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
          policy(self.obs_in)
        torch.cuda.current_stream(dev).wait_stream(side)
      self.graph = torch.cuda.CUDAGraph()
      with u._graph_capture():                                 # (the env's host counters are restored after the capture)
        with torch.cuda.graph(self.graph):
          prev = self.obs_in
          for t in range(self.T):
            if policy is not None:
              self.actions[t].copy_(policy(prev).to(torch.float32).reshape(n, A))
            if self._oob is not None:
              lo, hi = u._graph_bounds
              self._oob[t].copy_((~((self.actions[t] >= lo) & (self.actions[t] <= hi))).any(0))
              self.action_out_of_bounds[t].copy_(self._oob[t].any())
            u._graph_step(t, self.actions[t], {k: v[t] for k, v in self.out.items()}, self.clock.data_ptr())
            prev = self.obs[t]
          if policy is not None:
            self.obs_in.copy_(self.obs[self.T - 1])
    self.info = u._graph_info(self.out)

  def replay(self):
    """run the T captured steps (asynchronous, on torch's current stream) -> (obs, reward, done, info), each [T, N, ...]"""
    u = self.env
    for k, w in enumerate(u._graph_clock()):
      w = int(w) & (2**64 - 1)
      self.clock[k].fill_(w - (1 << 64) if w >= (1 << 63) else w)
    self.graph.replay()
    u._graph_advance(self.T, self.out)
    return self.obs, self.reward, self.done, self.info

  def check_actions(self):
    """synchronise and raise the reference's ValueError if an action of the last replay was out of bounds (minitaur_gym_env.py:276-281; the kernel clipped
    it to +-1.01 and stepped on).  Nothing to check for the envs whose reference clips silently."""
    if self._oob is None:
      return
    bad = self._oob.cpu()
    for t in range(self.T):
      if bool(bad[t].any()):
        raise ValueError('{}th action out of bounds.'.format(int(torch.nonzero(bad[t])[0])))

