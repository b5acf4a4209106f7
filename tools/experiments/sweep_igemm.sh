#!/bin/bash
# (tile, K split) candidates per shape in the harness; rank with sweep_table.py.  Build: tools/build_variant.sh ig_base --harness
for shp in "8 1024 1024 3" "16 768 768 3" "32 512 512 3" "16 1024 768 3" "64 256 256 3" "64 512 256 3" "32 768 512 3" "8 1024 1024 1" "16 768 768 1" "8 3072 1024 1" "8 1024 3072 1" "32 512 512 1" "32 1536 512 1" "16 2304 768 1"; do
  set -- $shp
  for big in 0 1; do for ks in 1 2 4 8 16 32; do
    timeout -k 5 60 ./build/ig_base $1 $2 $3 $big $ks 2 $4 | sed "s/^/ksize=$4 /"
  done; done
done
