#!/bin/bash
# Build: tools/build_variant.sh ig_base --harness
# Fixed vs per-K-step cost of the tiled conv kernel on the large maps: same map, growing Cin, statistics epilogue on/off.
cd "$(dirname "$0")/../.."
for H in 128 64 32; do
  for cin in 64 128 256 512 1024; do
    for st in 0 1; do
      for big in 0 1; do
        timeout -k 5 60 ./build/ig_base $H $cin 256 $big 1 2 3 $st 4 | grep gen
      done
    done
  done
done
