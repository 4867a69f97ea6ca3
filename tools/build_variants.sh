#!/bin/bash
# Builds compile-time variants of the library HERE (hipcc cross-compiles; the GPU box's minutes are for measuring): one shared
# object per variant under variants/, picked up on the box through MRS_SWARM_LIB.  usage: tools/build_variants.sh skin 0.5 0.75 1.0 ...
# (the unit list, the flags and the link line are mrs_multirotor_simulator_amd/build.py's, which also brings the regular objects up
# to date: a variant differs in the units named here)
set -e
mkdir -p variants
kind=$1; shift
for v in "$@"; do
  tag=$(echo "${kind}_$v" | tr -c 'A-Za-z0-9\n' '_')
  case $kind in
    skin) f=(--flags "collide.hip=-DMRS_SKIN=$v" --flags "collide_export.hip=-DMRS_SKIN=$v") ;;  # (both units see collide_work.h)
    collideflag) f=(--flags "collide.hip=$v" --flags "collide_export.hip=$v") ;;
    stepflag) f=(--flags "step_kernel_fast.hip=$v") ;;
    hostflag) f=(--flags "${v%% *}.hip=${v#* }") ;;  # "tick_sharded -DFOO=1": one host unit with extra flags
    *) echo "unknown kind: $kind" >&2; exit 2 ;;
  esac
  python -m mrs_multirotor_simulator_amd.build --out variants/libmrs_$tag.so "${f[@]}"
done
