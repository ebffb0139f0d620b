"""Multi-clip video-QA evaluation on cached encoder outputs.

Same result records and loss as the reference's `validate` (src/tasks/run_video_qa.py:225-276), but each batch's questions go
through the text encoder once and each clip through the visual encoder once.  The reference runs the whole model once per clip
(text encoder included) and pools the clips' logits on the host.  Here the fusion pass runs over the B*C (question, clip) pairs
with the question rows gathered by index, and alpro_clip_pool pools the logits and takes the answers on the device: one host copy
per batch.
"""
import torch

from alpro_amd import hip

SCORE_AGG_FUNCS = tuple(hip.POOL_MODES)   # run_video_qa.py:259-268


def _to(t, device):
    return t.to(device, non_blocking=True) if torch.is_tensor(t) and t.device != device else t


@torch.no_grad()
def inference_qa(model, batches, num_clips, num_frm, score_agg_func="mean", clip_chunk=32):
    """batches: iterable of the reference's validation batches -- dict(question_ids (list of B), visual_inputs (B, num_clips*num_frm, C, H, W),
    text_input_ids (B, Lt), text_input_mask (B, Lt), labels (B,) int64 or None); one question per video (the reference default).
    Returns (records, loss): records = [dict(question_id, answer)] with answer = the argmax of the pooled logits, as run_video_qa.py:270-276;
    loss = the sum over batches of each batch's clip-averaged cross-entropy (what the driver accumulates, :253-258; its valid/loss divides it
    by the number of questions), or None when the batches carry no labels.
    clip_chunk: clips per visual-encoder launch (bounds the activation memory at large B * num_clips)."""
    if score_agg_func not in SCORE_AGG_FUNCS:
        raise ValueError("Invalid value for pool_method, got %s, expect one of [`mean`, `max`, `lse`]" % score_agg_func)
    model.eval()
    device = next(model.parameters()).device
    records, loss = [], None
    C = int(num_clips)
    for batch in batches:
        qids = list(batch["question_ids"])
        B = len(qids)
        vis = _to(batch["visual_inputs"], device)
        clips = vis.view((B * C, num_frm) + tuple(vis.shape[2:]))          # row b*C + c = clip c of question b
        mask = _to(batch["text_input_mask"], device)
        text_embeds = model.encode_questions(_to(batch["text_input_ids"], device), mask)   # once per question, not once per clip
        if B * C <= clip_chunk:
            video_embeds = model.encode_clips(clips)
        else:
            video_embeds = None
            for s in range(0, B * C, clip_chunk):
                e = model.encode_clips(clips[s:s + clip_chunk])
                if video_embeds is None:
                    video_embeds = torch.empty((B * C,) + tuple(e.shape[1:]), dtype=e.dtype, device=e.device)
                video_embeds[s:s + e.shape[0]] = e
        vi = torch.arange(B * C, device=device)
        ti = torch.div(vi, C, rounding_mode="floor")
        labels = batch.get("labels")
        labels = _to(labels, device)[ti] if labels is not None else None
        logits, loss_rows = model.answer_logits(text_embeds, mask, video_embeds, ti, vi, labels)
        _, pred = hip.clip_pool(logits, C, score_agg_func)
        if labels is not None:
            # mean over the B*C pairs == the driver's (1/C) * sum over clips of each clip's batch-mean loss; shipped with the answers
            host = torch.cat([pred.to(torch.float64), loss_rows.mean().to(torch.float64).reshape(1)]).cpu()
            answers = host[:B].long().tolist()
            loss = (0.0 if loss is None else loss) + float(host[B])
        else:
            answers = pred.cpu().tolist()
        records.extend(dict(question_id=q, answer=a) for q, a in zip(qids, answers))
    return records, loss
