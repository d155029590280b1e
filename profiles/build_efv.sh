#!/bin/bash
# experiment build of the library with a variant of ONE source:  bash profiles/build_efv.sh <name> <source.hip> "<-D flags>"
# -> bsms-gnn_amd/lib_<name>.so.keep (the other objects come from the experiment build in _build_exp/)
set -e
cd "$(dirname "$0")/../bsms-gnn_amd"
name=$1; src=$2; flags=$3
mkdir -p _build_exp
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -DBSMS_EXPERIMENTS"
SRCS="plan rowsum chain chain_d32 chain_d64 chain_d96 chain_d128 chain_d160 chain_d192 chain_d224 chain_d256 efuse efwd wgrad gmp bsgmp optim hierarchy sim posgrad"
newer() { for h in csrc/chain.h csrc/chain_dev.h csrc/chain_kernels.h csrc/chain_edge.h csrc/chain_launch.h; do [ $h -nt $1 ] && return 0; done; return 1; }
for s in $SRCS; do
  f=csrc/$s.hip
  if [ ! -f _build_exp/$s.o ] || [ $f -nt _build_exp/$s.o ] || newer _build_exp/$s.o; then
    extra=""; { [ $s = rowsum ] || [ $s = sim ]; } && extra="-ffp-contract=off"
    /opt/rocm/bin/hipcc $F $extra -c $f -o _build_exp/$s.o &
  fi
done
wait
b=${src%.hip}
/opt/rocm/bin/hipcc $F $flags -c csrc/$b.hip -o _build_exp/${b}_$name.o
objs=""
for s in $SRCS; do
  if [ $s = $b ]; then objs="$objs _build_exp/${b}_$name.o"; else objs="$objs _build_exp/$s.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o lib_$name.so.keep $objs
echo "built lib_$name.so.keep ($src $flags)"
