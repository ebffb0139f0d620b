"""Video-QA fine-tuning step and multi-clip evaluation at the msrvtt_qa geometry, before / after the native QA path.

    python tools/qa_bench.py [--batch 12] [--frames 16] [--steps 10] [--warmup 3] [--rounds 3] [--eval-batch 12]

Step: AlproForSequenceClassification (1500 answers, 40-token questions, B x 16 frames x 224^2), fp16 operands + dynamic loss scaling,
FlatAdamW, train mode.  "after" = the model's forward (fusion input gathered, last fusion layer's tail on the [CLS] rows, _QAHead);
"before" = the previous path, restated below: torch.cat fusion input, every fusion row through the last layer, the answer MLP as two
_linear32 calls around F.relu, F.cross_entropy.  Both run on the same model and optimizer, alternated `rounds` times; each number is the
wall time of `steps` steps ending in a device synchronise, the median over the rounds is printed next to the spread.
Eval: alpro_amd.qa_eval.inference_qa (questions encoded once, clips once, pooled on the device) against the driver's loop
(run_video_qa.py:249-276: the whole model once per clip, logits copied to the host and pooled there), at C = 1 and 4 clips, questions/s.
Closed-form weights (tests/golden/det_init.py), so the two paths' outputs are compared too."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def legacy_logits(m, batch):
    """The parent revision's AlproForSequenceClassification._logits (torch.cat input, full fusion rows, eager ReLU between fp32 Linears)."""
    from alpro_amd.modeling.alpro_models import _linear32
    visual_inputs, mask = batch['visual_inputs'], batch['text_input_mask']
    text_embeds = m._text_embeds(batch['text_input_ids'], mask)
    image_embeds = m._forward_visual_embeds(visual_inputs)
    image_atts = torch.ones(image_embeds.size()[:-1], dtype=torch.long, device=visual_inputs.device)
    out = m._fusion(torch.cat([text_embeds, image_embeds], dim=1), torch.cat([mask, image_atts], dim=1))
    return _linear32(F.relu(_linear32(out[:, 0, :], m.classifier[0])), m.classifier[2])


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eval-batch", type=int, default=12)
    ap.add_argument("--eval-iters", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "qa_bench measures on the GPU"
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import AlproForSequenceClassification
    from alpro_amd.optim import FlatAdamW
    from alpro_amd.qa_eval import inference_qa
    from tests.conftest import BERT_CFG
    from tests.golden.det_init import det_batch, fill_state_dict_
    from tests.test_host_cpu import VENC, make_cfg
    B, T = args.batch, args.frames
    cfg = make_cfg(BERT_CFG, num_labels=1500, classifier="mlp", cls_hidden_scale=2, loss_type="ce")
    m = AlproForSequenceClassification(cfg, dict(VENC, num_frm=T))
    fill_state_dict_(m)
    m = m.cuda().train()
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in det_batch(B, T, Lt=40, seed_name="qa_bench", with_mlm=False, with_mpm=False).items()}
    batch["labels"] = (torch.arange(B, device="cuda") * 131) % 1500
    opt = FlatAdamW(m.parameters(), lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0, max_grad_norm=5.0)

    def step_after():
        opt.backward(m(batch)["loss"])
        opt.step()
        opt.zero_grad()

    def step_before():
        opt.backward(F.cross_entropy(legacy_logits(m, batch), batch["labels"]))
        opt.step()
        opt.zero_grad()

    print("# qa_bench: B=%d x %d frames x 224^2, Lt=40, 1500 answers, fp16 operands + loss scaling, FlatAdamW; %s" % (B, T, torch.cuda.get_device_name()))
    with rt.use_compute_dtype("fp16"):
        m.eval()
        with torch.no_grad():
            a, b = m(batch)["logits"], legacy_logits(m, batch)
        print("eval-mode logits |after - before| max %.3e (fp16 operands)" % (a.float() - b.float()).abs().max().item())
        m.train()
        for _ in range(args.warmup):
            step_before()
            step_after()
        res = {"before": [], "after": []}
        for _ in range(args.rounds):
            res["before"].append(timed(step_before, args.steps))
            res["after"].append(timed(step_after, args.steps))
        for k in ("before", "after"):
            v = res[k]
            print("step %-6s median %.2f ms  (rounds: %s)  %.1f questions/s" % (k, statistics.median(v) * 1e3, ", ".join("%.2f" % (x * 1e3) for x in v),
                                                                              B / statistics.median(v)))
        print("step speedup before/after: %.3fx" % (statistics.median(res["before"]) / statistics.median(res["after"])))

        m.eval()
        Be = args.eval_batch
        for C in (1, 4):
            eb = det_batch(Be, T * C, Lt=40, seed_name="qa_bench_eval", with_mlm=False, with_mpm=False)
            eb = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in eb.items()}
            eb["labels"] = (torch.arange(Be, device="cuda") * 37) % 1500
            eb["question_ids"] = list(range(Be))

            def native():
                return inference_qa(m, [eb], num_clips=C, num_frm=T, score_agg_func="mean")

            def driver():
                vis = eb["visual_inputs"].view((Be, C, T) + tuple(eb["visual_inputs"].shape[2:]))
                logits, losses = [], []
                with torch.no_grad():
                    for c in range(C):
                        out = m(dict(eb, visual_inputs=vis[:, c]))
                        logits.append(out["logits"].cpu())
                        losses.append(out["loss"].sum().item())
                return torch.stack(logits).mean(0).max(dim=-1)[1].tolist(), sum(losses) / C

            rec, loss = native()
            pred, dloss = driver()
            agree = sum(int(r["answer"] == p) for r, p in zip(rec, pred))
            tn, td = [], []
            for _ in range(args.rounds):
                td.append(timed(driver, args.eval_iters))
                tn.append(timed(native, args.eval_iters))
            qn, qd = Be / statistics.median(tn), Be / statistics.median(td)
            print("eval C=%d: inference_qa %.1f questions/s, driver loop %.1f questions/s (%.2fx); answers agree %d/%d, loss %.5f vs %.5f"
                  % (C, qn, qd, qn / qd, agree, Be, loss, dloss))


if __name__ == "__main__":
    main()
