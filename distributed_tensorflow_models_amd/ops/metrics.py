"""Streaming evaluation metrics: loss, top-1 / top-k, argmax accuracy, per-class counts, confusion matrix.

``StreamingMetrics`` adds every batch of an evaluation to one record and is read once at the end.  On the GPU an
``update`` is two launches on the current stream (csrc/kernels/metrics.hip) with nothing for the host to wait for;
``fetch()`` is the one synchronisation.  On the CPU the same definitions are written in torch ops.

Per row ``x = logits[r]``, ``t = labels[r]``:

* ``valid``: ``0 <= t < C``; an invalid row adds 1 to ``skipped`` and to nothing else.
* ``finite_row``: every logit of the row is finite.
* ``greater = #{c : x[c] > x[t]}``; ``in_top_k(k) = isfinite(x[t]) and greater < k`` (the rule of
  ``ops.elementwise.in_top_k``: ties at the boundary are in).  Counters ``top1`` and ``topk``.
* ``pred``: the argmax, lowest index among equal maxima (tf.argmax); ``argmax_correct`` counts ``pred == t``
  (tf.metrics.accuracy; differs from ``top1`` on ties).  Finite rows only.
* ``loss = log(sum_c exp(x[c] - m)) + m - x[t]``, ``m = max_c x[c]``: the exp-sum and its log in fp32, the last two
  terms added in fp64.  Finite rows only; each adds 1 to ``loss_rows``.
* a valid row that is not finite adds 1 to ``nonfinite``; it still counts in ``examples``, ``top1``, ``topk`` and
  ``support`` and in nothing else.

The record is one int64 vector: ``[examples, skipped, nonfinite, loss_rows, top1, topk, argmax_correct,
loss_sum (fp64 bits)]``, then ``support[C]``, ``top1_correct[C]``, ``predicted[C]`` and, with ``confusion=True``,
``confusion[C][C]`` (row = label, column = pred).  Integers are added with integer atomics or by a single writer
and ``loss_sum`` in a fixed order, so the record is bit-identical from run to run.
"""
import numpy as np
import torch

from . import _lib

HEADER = 8
_SCALARS = ("examples", "skipped", "nonfinite", "loss_rows", "top1", "topk", "argmax_correct")
MAX_CLASSES = 65536
MAX_CONFUSION_CLASSES = 4096
MAX_BATCH = 65536


def _ratio(a, b):
    return a / b if b else float("nan")


class StreamingMetrics:
    def __init__(self, num_classes, k=5, confusion=False, device="cpu"):
        C = int(num_classes)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError("num_classes %d outside [1, %d]" % (C, MAX_CLASSES))
        if not 1 <= int(k) <= C:
            raise ValueError("k = %d outside [1, num_classes = %d]" % (k, C))
        if confusion and C > MAX_CONFUSION_CLASSES:
            raise ValueError("a confusion matrix needs num_classes <= %d, got %d" % (MAX_CONFUSION_CLASSES, C))
        self.num_classes, self.k, self.confusion = C, int(k), bool(confusion)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            L = _lib.lib()
            assert L.dtm_metrics_header_words() == HEADER and L.dtm_metrics_max_classes() == MAX_CLASSES
            assert L.dtm_metrics_max_confusion_classes() == MAX_CONFUSION_CLASSES
            assert L.dtm_metrics_max_batch() == MAX_BATCH
        self._rec = torch.zeros(HEADER + 3 * C + (C * C if confusion else 0), dtype=torch.int64, device=self.device)
        self._rowloss = self._flags = None  # per-row scratch of the GPU pass, grown to the largest B seen

    # ---- accumulate ------------------------------------------------------------------------------------------
    def update(self, logits, labels):
        """Add one batch: ``logits`` [B, C] fp32 or bf16, ``labels`` [B] int32 or int64, both on ``self.device``."""
        C = self.num_classes
        if logits.dim() != 2 or logits.shape[1] != C:
            raise ValueError("logits %s: [B, %d] expected" % (tuple(logits.shape), C))
        B = logits.shape[0]
        if labels.dim() != 1 or labels.shape[0] != B:
            raise ValueError("labels %s: [%d] expected" % (tuple(labels.shape), B))
        if B > MAX_BATCH:
            raise ValueError("batch %d above the limit %d" % (B, MAX_BATCH))
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("logits: fp32 or bf16 expected, got %s" % logits.dtype)
        if labels.dtype not in (torch.int32, torch.int64):
            raise TypeError("labels: int32 or int64 expected, got %s" % labels.dtype)
        if logits.device != self._rec.device or labels.device != self._rec.device:
            raise ValueError("logits on %s, labels on %s, the record on %s"
                             % (logits.device, labels.device, self._rec.device))
        if B == 0:
            return
        if self.device.type == "cuda":
            self._update_gpu(logits, labels, B)
        else:
            self._update_cpu(logits, labels)

    def _update_gpu(self, logits, labels, B):
        if self._flags is None or self._flags.shape[0] < B:  # (the only allocation: first call at a larger B)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("StreamingMetrics.update(): first call at this batch size inside a hipGraph capture")
            self._rowloss = torch.empty(B, dtype=torch.float64, device=self.device)
            self._flags = torch.empty(B, dtype=torch.int32, device=self.device)
        if not logits.is_contiguous():  # (rows of a padded table: one copy; a contiguous view is read in place)
            logits = logits.contiguous()
        if not labels.is_contiguous():
            labels = labels.contiguous()
        rc = _lib.lib().dtm_eval_metrics(_lib.ptr(logits), 1 if logits.dtype == torch.bfloat16 else 0,
                                         _lib.ptr(labels), 1 if labels.dtype == torch.int64 else 0, B,
                                         self.num_classes, self.k, int(self.confusion), _lib.ptr(self._rec),
                                         _lib.ptr(self._rowloss), _lib.ptr(self._flags), _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError("dtm_eval_metrics failed (%d)" % rc)

    def _update_cpu(self, logits, labels):
        C, rec = self.num_classes, self._rec
        t = labels.long()
        valid = (t >= 0) & (t < C)
        rec[1] += int((~valid).sum())
        x, t = logits.float()[valid], t[valid]
        if x.shape[0] == 0:
            return
        xt = x.gather(1, t[:, None])[:, 0]
        greater = (x > xt[:, None]).sum(1)
        xt_fin = torch.isfinite(xt)
        top1, topk = xt_fin & (greater < 1), xt_fin & (greater < self.k)
        fin = torch.isfinite(x).all(1)
        rec[0] += x.shape[0]
        rec[2] += int((~fin).sum())
        rec[4] += int(top1.sum())
        rec[5] += int(topk.sum())
        cls = rec[HEADER:]
        cls[:C] += torch.bincount(t, minlength=C)
        cls[C:2 * C] += torch.bincount(t[top1], minlength=C)
        x, t, xt = x[fin], t[fin], xt[fin]
        if x.shape[0] == 0:
            return
        m = x.max(1).values
        # lowest index among the equal maxima
        pred = torch.where(x == m[:, None], torch.arange(C)[None, :], C).min(1).values
        loss = torch.log(torch.exp(x - m[:, None]).sum(1)).double() + (m.double() - xt.double())
        rec[3] += x.shape[0]
        rec[6] += int((pred == t).sum())
        rec[7:8].view(torch.float64).add_(loss.sum())
        cls[2 * C:3 * C] += torch.bincount(pred, minlength=C)
        if self.confusion:
            cls[3 * C:] += torch.bincount(t * C + pred, minlength=C * C)

    def reset(self):
        self._rec.zero_()

    def merge(self, process_group=None):
        """Sum the records of every rank of ``process_group`` (None: the default group) into this one: an
        all-gather of the packed record, then integers and ``loss_sum`` added in rank order, so every rank ends
        with the same bits."""
        import torch.distributed as dist
        world = dist.get_world_size(process_group)
        parts = [torch.empty_like(self._rec) for _ in range(world)]
        dist.all_gather(parts, self._rec, group=process_group)
        total = parts[0].clone()
        loss = total[7:8].view(torch.float64)
        for p in parts[1:]:  # rank order
            own = loss.clone()
            total += p
            loss.copy_(own + p[7:8].view(torch.float64))
        self._rec.copy_(total)

    # ---- read ------------------------------------------------------------------------------------------------
    def fetch(self):
        """The one synchronisation: the record as Python ints / floats and numpy int64 arrays, plus the derived
        ``mean_loss`` (loss_sum / loss_rows), ``precision_at_1`` and ``recall_at_k`` (top1, topk over examples),
        ``accuracy`` (argmax_correct over examples: a non-finite row has no prediction and counts as wrong),
        ``per_class_accuracy`` (top1_correct / support, NaN where support is 0) and ``mean_per_class_accuracy``
        over the classes with support.  Ratios with a zero denominator are NaN."""
        C = self.num_classes
        rec = self._rec.cpu().numpy()
        out = {n: int(rec[i]) for i, n in enumerate(_SCALARS)}
        out["loss_sum"] = float(rec[7:8].view(np.float64)[0])
        out["k"] = self.k
        cls = rec[HEADER:]
        out["support"] = cls[:C].copy()
        out["top1_correct"] = cls[C:2 * C].copy()
        out["predicted"] = cls[2 * C:3 * C].copy()
        if self.confusion:
            out["confusion"] = cls[3 * C:].reshape(C, C).copy()
        out["mean_loss"] = _ratio(out["loss_sum"], out["loss_rows"])
        out["precision_at_1"] = _ratio(out["top1"], out["examples"])
        out["recall_at_k"] = _ratio(out["topk"], out["examples"])
        out["accuracy"] = _ratio(out["argmax_correct"], out["examples"])
        has = out["support"] > 0
        pca = np.full(C, np.nan)
        pca[has] = out["top1_correct"][has] / out["support"][has]
        out["per_class_accuracy"] = pca
        out["mean_per_class_accuracy"] = float(pca[has].mean()) if has.any() else float("nan")
        return out
