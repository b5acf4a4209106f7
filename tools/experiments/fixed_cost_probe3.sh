#!/bin/bash
cd "$(dirname "$0")/../.."
BI_EMPTY=0 ./build/bi2 128 64 256 1 1 2 3 0 4 | grep kernel
for b in bi2 bi2DABL_EPI_NOSTORE bi2DABL_NOEPI; do
  for cin in 64 256; do
    echo -n "$b "; timeout -k 5 60 ./build/$b 128 $cin 256 1 1 2 3 0 4 | grep gen
    echo -n "$b "; timeout -k 5 60 ./build/$b 128 $cin 256 1 1 2 3 1 4 | grep gen
  done
  echo -n "$b "; timeout -k 5 60 ./build/$b 64 256 256 0 1 2 3 0 4 | grep gen
  echo -n "$b "; timeout -k 5 60 ./build/$b 64 64 256 0 1 2 3 0 4 | grep gen
  echo -n "$b "; timeout -k 5 60 ./build/$b 32 512 512 0 1 2 3 0 4 | grep gen
done
