#!/usr/bin/env bash
# Drop-in for the reference's run_scripts/infer.sh (which reads $model_name but sets "mdoel_name").
# One process per GPU: NGPU=8 bash run_scripts/infer.sh
model_name="${model_name:-${1:-}}"
exp_name="${exp_name:-${2:-zoomearth}}"
NGPU="${NGPU:-1}"
# ZE_THROUGHPUT=1: the fastest setting measured through this entry point on TIFF tiles on disk (README: 89.9 questions/s on one
# GPU) -- two engines per GPU with 512 chain slots each, the live chains of a lane holding while an admission round that leaves
# fewer than 384 of them live is still being prefilled (--hold) -- at the DEFAULT context budget of 4096 tokens per chain (2 x 77 GB of
# KV cache of the 288 GB): the stage-2 prompt of the real dataset reaches ~3200 tokens at the default image budgets, so a
# smaller --max_ctx would clip long chains (an error record instead of an answer) and change the accuracy.  bench.py's
# synthetic stream (L2 + N2 <= 1416 tokens) runs 2 x 768 slots of 2048 tokens; pass EXTRA_ARGS="--batch_size 768 --max_ctx 2048"
# only for prompts known to fit.  The default (64 chains, one engine) keeps a chain's output independent of the batch size
# for every --batch_size up to 64; above 64 the decode step runs on the row-streaming kernel family (same records for every
# size above 64, equal to the first family within bf16 rounding: DESIGN.md section 5).  EXTRA_ARGS are passed through (later
# flags win).
if [ "${ZE_THROUGHPUT:-0}" = "1" ]; then
  EXTRA_ARGS="--batch_size 512 --lanes 2 --hold 384 ${EXTRA_ARGS:-}"
fi
# ZE_DEVICE_TIFF=1: LZW / PackBits TIFF tiles are decoded on the GPU (--device_tiff_decode); other files keep the host decoder
if [ "${ZE_DEVICE_TIFF:-0}" = "1" ]; then
  EXTRA_ARGS="--device_tiff_decode ${EXTRA_ARGS:-}"
fi
echo "Infering model: $model_name on LRS-GRO!"
echo "Experiment name: $exp_name!"
if [ "$NGPU" -gt 1 ]; then
  python -m torch.distributed.run --nnodes=1 --nproc-per-node "$NGPU" --master-addr 127.0.0.1 --master-port "${MASTER_PORT:-29511}" \
    src/infer.py --model_name "$model_name" --exp_name "$exp_name" --steal ${EXTRA_ARGS:-}
  python -c "from zoomearth_amd.accel import merge_results; print(merge_results('results/$exp_name', $NGPU, 'results/$exp_name.jsonl'), 'records merged')"
else
  python src/infer.py --model_name "$model_name" --exp_name "$exp_name" ${EXTRA_ARGS:-}
fi
