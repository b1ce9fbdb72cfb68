"""What tests/test_policy_bf16.py (no GPU) and tests/test_policy_bf16_gpu.py share (a plain module: no tests, no fixtures): the float32 values whose rounding to
bf16 the packing test pins, networks that carry them, and the env widths."""
import numpy as np
import torch

WIDTHS = {'door': (14, 4), 'peg': (14, 4), 'minitaur': (32, 8), 'kitchen': (46, 9)}

# (float32 bit pattern, the bf16 bit pattern round-to-nearest-even gives): +-0; the largest float32 below 2 (rounds UP into the next binade); two ties (the kept bits
# even: down; odd: up to the even neighbour); one bit above and one below a tie; the smallest bf16 subnormal, and a float32 subnormal that rounds to it; the largest finite bf16
SPECIAL = [(0x00000000, 0x0000), (0x80000000, 0x8000), (0x3FFFFFFF, 0x4000), (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F808001, 0x3F81), (0xBF817FFF, 0xBF81),
           (0x00010000, 0x0001), (0x0000C000, 0x0001), (0x7F7F0000, 0x7F7F)]


def special_f32():
  return np.array([b for b, _ in SPECIAL], np.uint32).view(np.float32).copy()


def special_bf16_bits():
  return np.array([w for _, w in SPECIAL], np.uint16)


def bits16(t):
  """a bf16 tensor's bit patterns as a numpy uint16 array"""
  return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def plant_specials(layers):
  """the special values at the head of the first and of the last row of the FIRST layer's weights, in place (one value of bf16's largest magnitude per row: the row's
  sum stays a number, and a tanh hidden layer bounds it) -> layers"""
  w0 = layers[0][0]
  s = special_f32()
  k = min(len(s), w0.shape[1])
  w0[0, :k] = s[-k:]                                      # (a narrow input keeps the tail: the subnormals and the largest finite value)
  w0[-1, :k] = s[-k:][::-1]
  return layers
