#!/bin/bash
# The one script that compiles a variant of the library or of the conv harness (for same-box A/B runs: tools/ab_libs.sh).
#   tools/build_variant.sh NAME [--patch FILE]... [--harness] [extra hipcc flags...]
# -> build/lib_NAME.so, or with --harness build/NAME from tools/bench_igemm.hip.  The sources are copied to a temporary
# directory and the patches (tools/experiments/probes/) applied THERE, never to the tree; source list and compiler flags
# are those of the product build (ishapediting_amd/build.py: SOURCES, FLAGS).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
patches=(); harness=0; extra=()
while [ $# -gt 0 ]; do
  case $1 in
    --patch) patches+=("$(realpath "$2")"); shift 2;;
    --harness) harness=1; shift;;
    *) extra+=("$1"); shift;;
  esac
done
T=$(mktemp -d); trap 'rm -rf $T' EXIT
mkdir -p $T/ishapediting_amd $T/tools $R/build
cp -r $R/ishapediting_amd/csrc $T/ishapediting_amd/ && rm -rf $T/ishapediting_amd/csrc/build
cp -r $R/include $T/ && cp $R/tools/bench_igemm.hip $T/tools/
for p in "${patches[@]}"; do
  patch -d $T -p1 --no-backup-if-mismatch < "$p" || { echo "build_variant: $p does not apply to these sources" >&2; exit 1; }
done
cd $R
FLAGS=$(python -c "import ishapediting_amd.build as b; print(' '.join(b.FLAGS))")
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ $harness = 1 ]; then
  $HIPCC $FLAGS "${extra[@]}" $T/tools/bench_igemm.hip -o build/$name
  ls -la build/$name
else
  python -c "import ishapediting_amd.build as b; print('\n'.join(b.SOURCES))" |
    xargs -P 6 -I{} bash -c "s={}; $HIPCC $FLAGS ${extra[*]} -c $T/ishapediting_amd/csrc/\$s -o $T/\${s%.hip}.o"
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o build/lib_$name.so $T/*.o
  ls -la build/lib_$name.so
fi
