#!/bin/bash
# Refresh the persisted GEMM tile table (construction-clip_amd/cclip_hip/gemm_tune.json) on a GPU box, from the repository root:
#   OUT=<dir> bash tools/tune_gemm.sh      then      cp <dir>/gemm_tune.json construction-clip_amd/cclip_hip/      (OUT default: tool_out)
# Every workload bench.py knows is run once with CCLIP_TUNE_FILE set, so every (shape, layout, epilogue) key the hot path
# issues is timed once and written; keys are tied to the kernel-source hash (cclip_hip/ops.py:kernel_source_hash).
# --full: the roofline leg runs the step on one stream and encode_image on the whole batch, shapes the table must hold too.
set -e
O=${OUT:-tool_out}
mkdir -p "$O"
export CCLIP_TUNE_FILE=$(cd "$O" && pwd)/gemm_tune.json
export CCLIP_TUNE_EXACT=1      # time every shape these runs meet (no nearest-shape fallback)
export CCLIP_PACK_TEXT=0       # the table holds the dense text shapes; packed batches take the nearest entry
cp -f construction-clip_amd/cclip_hip/gemm_tune.json "$CCLIP_TUNE_FILE" 2>/dev/null || true
python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras > "$O"/tune_train_bf16.log 2>&1
# the packed text tower's shapes for the default synthetic batch (about half the dense rows): other packed batches take the nearest
CCLIP_PACK_TEXT=1 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras > "$O"/tune_train_bf16_packed.log 2>&1
CCLIP_PACK_TEXT=1 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --dtype fp16 > "$O"/tune_train_fp16_packed.log 2>&1
python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras --dtype fp16 > "$O"/tune_train_fp16.log 2>&1
python bench.py --full --mode image --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tune_image.log 2>&1
python bench.py --full --mode fwd --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tune_fwd.log 2>&1
python bench.py --full --mode caption --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tune_caption.log 2>&1
CCLIP_PACK_TEXT=1 python bench.py --full --mode caption --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tune_caption_packed.log 2>&1
python bench.py --full --mode image --model ViT-L/14@336px --batch 256 --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tune_l14.log 2>&1
python - <<'PY'
import json, os
t = json.load(open(os.environ["CCLIP_TUNE_FILE"]))
print("entries:", len(t["table"]), "hash:", t["kernel_source_hash"])
PY
