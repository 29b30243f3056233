"""Training-side TensorBoard summaries beyond the scalars (reference cnn/cifar10.py:104-121,375-381,
cnn/cifar10_input.py:139):

* ``--summary_histograms``   ``<var>`` and ``<var>/gradients`` histograms of every trainable variable
* ``--summary_activations``  ``<end_point>/activations`` histograms and ``<end_point>/sparsity`` scalars
* ``--summary_images N``     ``images/image/<i>`` of the current input batch

``launch()`` enqueues the device work of a summary step right after the training step (ops.summary.TensorStats:
two launches for all variables and gradients, two more for the activations, a few torch ops for the images) and
starts the copies into pinned host memory; ``write()`` runs after the trainer's own device synchronisation of that
logged step and puts every value into ONE event.  Neither adds a synchronisation.

Variables are read AFTER the step's update (the flat gradient buffer keeps its values until the next zero_grad,
the weights do not keep theirs), so a ``<var>`` histogram at global step g shows the weights that step g produced.
Gradients exist under BSP only (scale: the data-parallel 1/W); ASP / SSP replicas get the variable histograms of
their local replica and no gradient histograms.
"""
import inspect

import numpy as np
import torch

from ..compat import logging
from ..ops.summary import TensorStats
from . import tb


def images_to_uint8(images):
    """[N, H, W, C] float (or uint8, passed through) -> uint8, per image: with a finite minimum below 0 the image
    maps to 128 + x * 127 / max|x|, otherwise to x * 255 / max; the scale is 0 when that maximum is 0; the result is
    clamped to [0, 255] and truncated.  A pixel with a non-finite channel becomes red ((255, 0, 0, 255) cut to C
    channels).  This is the project's statement of TF-1's tf.summary.image rule."""
    if images.dtype == torch.uint8:
        return images
    x = images.float()
    fin = torch.isfinite(x)
    big = torch.finfo(torch.float32).max
    mn = torch.where(fin, x, torch.full_like(x, big)).amin(dim=(1, 2, 3), keepdim=True)
    mx = torch.where(fin, x, torch.full_like(x, -big)).amax(dim=(1, 2, 3), keepdim=True)
    neg = mn < 0
    amax = torch.maximum(mn.abs(), mx.abs())
    zero = torch.zeros_like(mn)
    scale = torch.where(neg, torch.where(amax > 0, 127.0 / amax, zero), torch.where(mx > 0, 255.0 / mx, zero))
    offset = torch.where(neg, torch.full_like(mn, 128.0), zero)
    y = (torch.where(fin, x, torch.zeros_like(x)) * scale + offset).clamp(0, 255).to(torch.uint8)
    bad = ~fin.all(dim=-1, keepdim=True)
    red = torch.tensor([255, 0, 0, 255][:x.shape[-1]], dtype=torch.uint8, device=x.device)
    return torch.where(bad, red, y)


class TrainSummaries:
    def __init__(self, model, step_fn, mode, histograms=False, activations=False, images=0):
        self.model = model
        self.mode = mode
        self.histograms, self.activations, self.num_images = bool(histograms), bool(activations), int(images)
        self.dp = getattr(step_fn, "dp", None) if mode == "bsp" else None
        self._var_stats, self._var_key, self._var_tags = None, None, []
        self._act, self._act_done = None, None  # (_act_done: the last fetched activation pass, for its pinned buffers)
        self._img, self._img_host = None, None
        self._warned = set()
        self._launched = False
        if self.activations and "end_points" not in inspect.signature(model.forward).parameters:
            logging.warning("--summary_activations: %s takes no end_points, no activation summaries",
                            type(model).__name__)
            self.activations = False

    # ---- device side (after the training step, before the logged step's synchronisation) -------------------
    def _variable_rows(self):
        tags, tensors, scales = [], [], []
        params = [p for p in self.model.parameters() if p.requires_grad and getattr(p, "tf_name", None)]
        for p in params:
            tags.append(p.tf_name)
            tensors.append(p.detach())
            scales.append(1.0)
        if self.dp is not None:
            for p in params:
                g = getattr(p, "main_grad", None)
                if g is not None:
                    tags.append(p.tf_name + "/gradients")
                    tensors.append(g)
                    scales.append(self.dp.grad_scale)
        return tags, tensors, scales

    def _end_points(self, images):
        """One extra training-mode forward under no_grad with end_points; the BN moving statistics and the dropout
        / RNG streams are put back, so the training run is bit-identical with and without it."""
        from ..engine import side_forward
        from ..ops.lazy import as_tensor
        ep = {}
        with side_forward(self.model, images.device, rng=True), torch.no_grad():
            self.model(images, training=True, end_points=ep)
            ep = {k: as_tensor(v) for k, v in ep.items()}
        out = {}
        for k, v in ep.items():
            if isinstance(v, torch.Tensor) and v.numel() and v.is_floating_point():
                if v.dtype not in (torch.float32, torch.bfloat16):
                    v = v.float()
                out[k] = v.contiguous()
        return out

    def launch(self, images):
        if self.histograms:
            tags, tensors, scales = self._variable_rows()
            key = tuple(t.data_ptr() for t in tensors)
            if tensors and key != self._var_key:  # tables are built once; again only if a tensor moved
                self._var_stats, self._var_key, self._var_tags = TensorStats(tensors, scales), key, tags
            if self._var_stats is not None:
                self._var_stats.launch()
        if self.activations:
            ep = self._end_points(images)
            self._act = None
            if ep:  # fresh allocations every step: the table is rebuilt
                st = TensorStats(list(ep.values()), pinned_from=self._act_done)
                st.launch()
                self._act = (list(ep.keys()), st)
        if self.num_images > 0:
            u8 = images_to_uint8(images[:self.num_images].detach())
            if u8.is_cuda:
                if self._img_host is None or self._img_host.shape != u8.shape:  # pinned once, reused
                    self._img_host = torch.empty(u8.shape, dtype=torch.uint8).pin_memory()
                self._img_host.copy_(u8, non_blocking=True)
                u8 = self._img_host
            self._img = u8
        self._launched = True

    # ---- host side (after the synchronisation) ----------------------------------------------------------
    def _histo(self, values, tag, rec):
        if rec["nonfinite"] > 0:
            if tag not in self._warned:
                self._warned.add(tag)
                logging.warning("summary %s: %d non-finite of %d values, histogram skipped", tag, rec["nonfinite"],
                                rec["n"])
            return
        values.append(tb.histogram_value(tag, rec))

    def write(self, writer, step):
        if not self._launched:
            return
        self._launched = False
        values = []
        if self.histograms and self._var_stats is not None:
            for tag, rec in zip(self._var_tags, self._var_stats.fetch()):
                self._histo(values, tag, rec)
        if self.activations and self._act is not None:
            names, st = self._act
            for name, rec in zip(names, st.fetch()):
                self._histo(values, name + "/activations", rec)
                values.append(tb.scalar_value(name + "/sparsity", rec["zeros"] / float(rec["n"])))
            st.release()
            self._act, self._act_done = None, st
        if self._img is not None:
            imgs = np.asarray(self._img.numpy())
            for i in range(imgs.shape[0]):
                values.append(tb.image_value("images/image/%d" % i if imgs.shape[0] > 1 else "images/image", imgs[i]))
            self._img = None
        writer.add_summaries(values, step)
