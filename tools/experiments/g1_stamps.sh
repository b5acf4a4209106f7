#!/bin/bash
# stamp tables of the 1x1 GEMMs of the attention blocks.  Build: tools/build_variant.sh ig_stamps --harness -DISHAP_STAMPS
cd "$(dirname "$0")/../.."
for shape in "32 512 512 0 1 2 1 0 8" "32 512 1536 0 1 2 1 0 8" "16 768 2304 0 1 2 1 0 8" "16 768 768 0 1 2 1 0 8"; do
  echo "== $shape"; timeout -k 5 60 build/ig_stamps $shape | tail -14
done
