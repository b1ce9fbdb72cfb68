#!/bin/bash
# build tools/ubench/libearl_policy_stamped.so = the shipped library with tabletop_policy.hip, tabletop_policy_gaussian.hip and tabletop_policy_pair.hip recompiled under
# -DEARL_POLICY_STAMPS (per-phase s_memtime stamps of the closed-loop policy kernel, csrc/tabletop_policy.h; read by tools/prof_policy.py, each unit through
# its own reader).  Needs the shipped objects (make -C earl_benchmark_amd/csrc); their list is the Makefile's (`make print-objects`), less the three stamped units.
set -e
cd "$(dirname "$0")/../earl_benchmark_amd/csrc"
FLAGS="-DEARL_POLICY_STAMPS --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fPIC"
OUT=../../tools/ubench
STAMPED="tabletop_policy tabletop_policy_gaussian tabletop_policy_pair"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OBJS=
mkdir -p $OUT
SHIPPED=$(make -s print-objects)
for u in $STAMPED; do
  $HIPCC $FLAGS -c -o $OUT/${u}_stamped.o $u.hip
  SHIPPED=$(echo " $SHIPPED " | sed "s/ $u\.o / /")
  OBJS="$OBJS $OUT/${u}_stamped.o"
done
$HIPCC $FLAGS -shared -o $OUT/libearl_policy_stamped.so $OBJS $SHIPPED
rm -f $OBJS
echo built libearl_policy_stamped.so
