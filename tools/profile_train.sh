# rocprofv3 kernel-trace summaries of the default and the single-stream train step (run on the GPU box via gpurun; copies go to profiles/)
set -e
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT:-$R/tool_out}      # output folder (absolute)
mkdir -p "$O"
rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_default -- python3 "$R"/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > "$O"/prof_default.log 2>&1
export CCLIP_WGRAD_STREAM=0
rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_single -- python3 "$R"/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --tower-streams 1 > "$O"/prof_single.log 2>&1
