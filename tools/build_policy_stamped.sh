#!/bin/bash
# build tools/ubench/libearl_policy_stamped.so = the shipped library with tabletop_policy.hip, tabletop_policy_gaussian.hip and tabletop_policy_pair.hip recompiled under
# -DEARL_POLICY_STAMPS (per-phase s_memtime stamps of the closed-loop policy kernel, csrc/tabletop_policy.h; read by tools/prof_policy.py, each unit through
# its own reader).  Needs the shipped objects (make -C earl_benchmark_amd/csrc).
set -e
cd "$(dirname "$0")/../earl_benchmark_amd/csrc"
FLAGS="-DEARL_POLICY_STAMPS --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fPIC"
mkdir -p ../../tools/ubench
/opt/rocm/bin/hipcc $FLAGS -c -o ../../tools/ubench/tabletop_policy_stamped.o tabletop_policy.hip
/opt/rocm/bin/hipcc $FLAGS -c -o ../../tools/ubench/tabletop_policy_gaussian_stamped.o tabletop_policy_gaussian.hip
/opt/rocm/bin/hipcc $FLAGS -c -o ../../tools/ubench/tabletop_policy_pair_stamped.o tabletop_policy_pair.hip
/opt/rocm/bin/hipcc $FLAGS -shared -o ../../tools/ubench/libearl_policy_stamped.so ../../tools/ubench/tabletop_policy_stamped.o ../../tools/ubench/tabletop_policy_gaussian_stamped.o ../../tools/ubench/tabletop_policy_pair_stamped.o tabletop_policy_population.o tabletop3_policy.o tabletop3_pair.o tabletop3_eval.o tabletop_branch.o tabletop_plan.o tabletop_mpc.o tabletop_plan_value.o tabletop_mpc_value.o tabletop.o glue.o physics.o physics_w8.o physics_mt.o physics_l64.o physics_kitchen.o physics_kitchen_policy.o physics_bf16.o physics_w8_bf16.o physics_mt_bf16.o physics_kitchen_policy_bf16.o
rm -f ../../tools/ubench/tabletop_policy_stamped.o ../../tools/ubench/tabletop_policy_gaussian_stamped.o ../../tools/ubench/tabletop_policy_pair_stamped.o
echo built libearl_policy_stamped.so
