#!/bin/bash
# Profile the default bench command on the GPU box: kernel-trace stats into gpurun_out/prof_<tag>/
set -o pipefail
tag=${1:-r1}
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
mkdir -p gpurun_out/prof_$tag
out=$_  # the directory made above
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out -o bench -- python3 bench.py --full > $out/bench.json 2> $out/bench.err
