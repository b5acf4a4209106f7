#!/bin/bash
# statistics cost of the staged epilogue: no statistics / one table / 8 / 32 copies of the table (harness, warm; wrong statistics by design).
# Builds: tools/build_variant.sh ig_base --harness; tools/build_variant.sh ig_stat8 --harness --patch tools/experiments/probes/stat_copies.patch
# -DABL_STAT_COPIES=8 (ig_stat32: =32).  Result: profiles/round3_stat_copies.txt
cd "$(dirname "$0")/../.."
for b in ig_base ig_stat8 ig_stat32; do
  for st in 0 1; do
    echo -n "$b stats=$st "; timeout -k 5 60 ./build/$b 128 256 256 1 1 2 3 $st 4 | grep gen
    echo -n "$b stats=$st "; timeout -k 5 60 ./build/$b 64 256 256 0 1 2 3 $st 4 | grep gen
    echo -n "$b stats=$st "; timeout -k 5 60 ./build/$b 64 512 256 0 1 2 3 $st 4 | grep gen
  done
done
