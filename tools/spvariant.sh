#!/bin/bash
# Diagnostic builds of the one-pod path (ksched_spread.hip) with extra defines:
#   tools/spvariant.sh NAME "-DKS_..."  ->  k8s-1m_amd/ksched/lib/NAME/libksched.so
# (load with KSCHED_LIB_DIR; never used by tests / bench / smoke)
set -e
cd "$(dirname "$0")/../k8s-1m_amd"
# the product's other objects, as the Makefile names and builds them
OBJS="$(make -s print-KERNEL_OBJS | tr ' ' '\n' | grep -v ksched_spread.o | tr '\n' ' ') $(make -s print-HOST_OBJS)"
make -s $OBJS
NAME=$1; shift
mkdir -p ksched/lib/$NAME
F="-O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -Wall -I../include -Icsrc"
/opt/rocm/bin/hipcc $F "$@" -c csrc/ksched_spread.hip -o build/ksched_spread_$NAME.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ksched/lib/$NAME/libksched.so \
  build/ksched_spread_$NAME.o $OBJS -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
