"""Bulk captioning over the MI355X engine: the command line of the reference's scripts/caption_bulk.py (same arguments, same output
files), batched across proteins (`--batch_size`).  See procyon_amd/pipelines.py.

Like the reference script it generates with the model AS LOADED (fp32 checkpoint -> fp32 arithmetic, /root/reference/scripts/caption_bulk.py:70-73):
the fp32 operator family with its cached decode step -- a compatibility path, one launch per operator: 82 ms per 10-row step at 512 cached
tokens (profiles/decode_f32_ab.log), about 20 x the bf16 engine's 3.9 ms.  `--fp32_stream` keeps fp32 and runs every cached step
on the device-resident fp32 step: 9.3 ms for the same step, 8.9 x faster than the operator path.  `--fp32_device` runs the
beam search's selection on the device as well (one prefill per protein, no host round trip per step).  `--bf16` casts the model first,
as the evaluation framework and the retrieval service do (evaluate/framework/procyon.py:64-65): the fused bf16 engine."""
import argparse

import pandas as pd
import torch

from procyon.model.model_unified import UnifiedProCyon
from procyon.training.train_utils import set_seed
from procyon_amd.pipelines import caption_bulk, chunk_rows


def main(args):
    device = torch.device("cuda")
    data_args, model_args, _ = UnifiedProCyon.get_checkpoint_configs(resume_from_checkpoint=args.ckpt)
    model, _ = UnifiedProCyon.from_pretrained(checkpoint_dir=args.ckpt)
    if sum(map(bool, (args.bf16, args.fp32_stream, args.fp32_device))) > 1:
        raise SystemExit("caption_bulk: --fp32_stream and --fp32_device choose the decode step of the fp32 model, --bf16 casts it: pass one of them")
    if args.bf16:
        model.bfloat16()
    elif args.fp32_device:
        print("caption_bulk: running in fp32 like the reference script, the beam search entirely on the device (one prefill per protein, one "
              "replayed launch chain per step: the fp32 step, the beam step and the K / V reorder of the generated suffix)", flush=True)
    elif args.fp32_stream:
        print("caption_bulk: running in fp32 like the reference script, the cached steps on the device-resident fp32 step (one replayed graph per "
              "step; measured 9.3 ms per 10-row step at 512 cached tokens against 82 ms of the operator path, about 2.4 x the bf16 engine's step)",
              flush=True)
    else:
        print("caption_bulk: running in fp32 like the reference script (one launch per operator, a host round trip per step: measured 82 ms per "
              "10-row step at 512 cached tokens, about 20 x the fused bf16 engine of --bf16 and 8.9 x the fp32 step of --fp32_stream)", flush=True)
    model.to(device)
    model.eval()
    set_seed(1234)
    table = pd.read_csv(args.uniprot_id_file)
    start, end = chunk_rows(table.shape[0], args.num_chunks, args.chunk_idx, "caption_bulk")
    df = caption_bulk(model, model_args, data_args, table["uniprot_id"].iloc[start:end].tolist(), args.prompt_dataset, args.prompt_relation,
                      args.max_len, args.beam_size, args.diversity_penalty, args.save_path, args.batch_size, device=device,
                      **({"decode_f32": "device"} if args.fp32_device else {"decode_f32": "stream"} if args.fp32_stream else {}),
                      **({"stop_on_eos": True} if args.stop_on_eos else {}))
    print(df)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", required=True, help="Path to ProCyon checkpoint")
    p.add_argument("--save_path", default=None, type=str, help="CSV file name to save captions to")
    p.add_argument("--chunk_idx", default=None, type=int)
    p.add_argument("--num_chunks", default=None, type=int)
    p.add_argument("--uniprot_id_file", required=True, type=str, help="CSV with a uniprot_id column")
    p.add_argument("--prompt_dataset", default="uniprot")
    p.add_argument("--prompt_relation", default="all")
    p.add_argument("--beam_size", default=10, type=int)
    p.add_argument("--max_len", default=200, type=int)
    p.add_argument("--diversity_penalty", default=0.8, type=float)
    p.add_argument("--bf16", action="store_true", help="cast the model to bfloat16 first (the fused engine; the reference script runs fp32)")
    p.add_argument("--fp32_stream", action="store_true", help="keep fp32 and run the cached decode steps on the device-resident fp32 step "
                                                              "(generate(decode_f32='stream'), DESIGN.md 4.10)")
    p.add_argument("--fp32_device", action="store_true", help="keep fp32 and run the beam search entirely on the device: the fp32 step and the "
                                                              "selection (generate(decode_f32='device'), DESIGN.md 4.10a)")
    p.add_argument("--stop_on_eos", action="store_true", help="end every generation where its text ends (caption_bulk(stop_on_eos=True), "
                                                              "DESIGN.md 4.11; the beam search of this script already does)")
    p.add_argument("--batch_size", default=8, type=int, help="proteins per engine call (the reference script: 1)")
    main(p.parse_args())
