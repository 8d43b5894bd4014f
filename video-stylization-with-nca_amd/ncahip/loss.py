"""Training objective for ConditionedNCATrainer (reference: EncoderConditioning/loss/loss.py:17-76).

In scope here: the overflow term (loss.py:37-40), exact.  The VGG16 appearance / content terms are the
"next" row f2 of SURVEY.md section 8: torchvision and the ImageNet weights are not available offline, so the
feature extractor below is a pure-torch VGG16-features definition that loads a local `vgg16-397923af.pth`
when NCAHIP_VGG16_WEIGHTS points at one and otherwise runs with seeded random weights (timing stand-in;
loss values vs the reference are then "parity unpinned").  Appearance types: 'OT' (the reference's default: relaxed
EMD over cosine distances + first/second moment matching, appearance_loss.py:149-220), 'Gram' and 'SlW' (sliced
Wasserstein, project-sort over the image + the five style levels, appearance_loss.py:109-140).  The OT arithmetic itself is
pinned by tests/test_trainer_logic.py against an independent float64 evaluation of the same formulas; the batch is evaluated
with batched matrix products (`ot_loss_batched`) instead of the reference's per-sample Python loop (:212-220) -- same index
draws from numpy's global stream in the same order, same value up to summation order.  `feature_dtype=torch.bfloat16` runs the
VGG convolutions in bf16 on the device (BASELINE configs[2]); the loss arithmetic on the features stays fp32.
"""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

_VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
STYLE_LAYERS = (1, 6, 11, 18, 25)   # appearance_loss.py:85,114,144
CONTENT_LAYER = 19                  # content_loss.py:17 (conv4_2 pre-ReLU index in torchvision's features)


class VGG16Features(nn.Module):
    def __init__(self):
        super().__init__()
        layers, c = [], 3
        for v in _VGG_CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(c, v, 3, padding=1), nn.ReLU(inplace=False)]
                c = v
        self.features = nn.Sequential(*layers)
        path = os.environ.get("NCAHIP_VGG16_WEIGHTS", "")
        if path and os.path.exists(path):
            sd = torch.load(path, weights_only=True)
            self.load_state_dict({k: v for k, v in sd.items() if k.startswith("features.")})
            self.pinned = True
        else:
            g = torch.Generator().manual_seed(16)
            with torch.no_grad():
                for m in self.features:
                    if isinstance(m, nn.Conv2d):
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (m.weight[0].numel())) ** 0.5)
                        m.bias.zero_()
            self.pinned = False
            warnings.warn("ncahip.loss: no VGG16 weights (NCAHIP_VGG16_WEIGHTS); using seeded random features -- "
                          "appearance/content loss values are not comparable with the reference")
        for p in self.parameters():
            p.requires_grad_(False)
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406])[None, :, None, None])
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225])[None, :, None, None])

    def forward(self, x, layers):
        x = (x - self.mean) / self.std
        dt = self.features[0].weight.dtype          # bf16 when the module was cast (.to(torch.bfloat16)): convs on bf16 MFMA
        x = x.to(dt)
        if self.features[0].weight.is_contiguous(memory_format=torch.channels_last) and not self.features[0].weight.is_contiguous():
            x = x.contiguous(memory_format=torch.channels_last)     # NHWC convolutions (Loss(channels_last=True))
        out, last = {}, max(layers)
        for i, m in enumerate(self.features):
            x = m(x)
            if i in layers:
                out[i] = x.float()
            if i >= last:
                break
        return out


def _gram(f):
    b, c, h, w = f.shape
    f = f.reshape(b, c, h * w)
    return f @ f.transpose(1, 2) / (h * w)


def _sliced_wasserstein(source, target, n_proj=32):
    """appearance_loss.py:121-136: source [b,c,n], target [1,c,m] flattened features; random unit projections drawn on the
    CPU generator (torch.randn(ch, 32)), project + sort, nearest-resample the target to n, SUM of squared differences."""
    ch, n = source.shape[-2:]
    proj = F.normalize(torch.randn(ch, n_proj), dim=0).to(source.device)
    ps = torch.einsum("bcn,cp->bpn", source, proj).sort()[0]
    pt = torch.einsum("bcn,cp->bpn", target, proj).sort()[0]
    return (ps - F.interpolate(pt, n, mode="nearest")).square().sum()


def sliced_wasserstein_fused(source, target, n_proj=32):
    """_sliced_wasserstein on this library's kernels (csrc/nca_slw.hip): the same torch.randn(ch, 32) draw on the CPU generator, so
    torch's CPU RNG stream is left exactly where the torch path leaves it; projection, a stable segmented sort of (key, index)
    pairs, the nearest resample of the target through a cached index map (F.interpolate applied to an arange), the sum of squares
    and the closed-form backward (scatter through the sort's permutation, then proj . dk) all run as HIP kernels.  Only
    n_proj == 32; CUDA float32 features only (no CPU fallback); c = 3 or a multiple of 4 up to 512.

    A level whose rows are longer than 65 536 positions (source or target) is taken on the torch path, level by level, with the
    projection already drawn: the sort kernels cover rows up to 65 536.  Non-finite features are outside the contract.  Equal
    keys are ordered by position (a stable sort); the loss value does not depend on that order, the gradient's assignment of
    equal keys does."""
    from . import ops
    from .autograd import SlicedWasserstein
    if n_proj != ops.SLW_DIRECTIONS:
        raise ValueError(f"ncahip.loss: sliced_wasserstein_fused covers n_proj == {ops.SLW_DIRECTIONS}, got {n_proj}")
    ch, n = source.shape[-2:]
    m = target.shape[-1]
    proj = F.normalize(torch.randn(ch, n_proj), dim=0).to(source.device)
    if n > ops.SLW_MAX_LEN or m > ops.SLW_MAX_LEN:
        ps = torch.einsum("bcn,cp->bpn", source, proj).sort()[0]
        pt = torch.einsum("bcn,cp->bpn", target, proj).sort()[0]
        return (ps - F.interpolate(pt, n, mode="nearest")).square().sum()
    if not source.is_cuda:
        ops._dev(source, "source")                          # raises: no CPU fallback
    return SlicedWasserstein.apply(source, target, proj, ops.slw_index_map(m, n, source.device))


_SLW_IMPLS = {"torch": _sliced_wasserstein, "fused": sliced_wasserstein_fused}


def _to_nchw(img) -> torch.Tensor:
    """appearance_loss.py:41-43 (torchvision ToTensor + unsqueeze): a PIL image or an H x W x C uint8 array becomes a
    [1,C,H,W] float tensor in [0,1]; float arrays are only transposed; a float tensor is taken as C x H x W (or N x C x H x W)
    already in network range."""
    if isinstance(img, torch.Tensor):
        t = img.float()
        return t[None] if t.dim() == 3 else t
    if not isinstance(img, np.ndarray):          # PIL.Image (or anything exposing the array interface)
        img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))
    t = t.float().div(255.0) if img.dtype == np.uint8 else t.float()
    return t[None]


def _pairwise_cos(x, y):
    """appearance_loss.py:150-156: 1 - <x_i, y_j> / (|x_i| + 1e-10) / (|y_j| + 1e-10), x [N,d], y [M,d]."""
    xn = torch.sqrt((x ** 2).sum(1)).view(-1, 1)
    yn = torch.sqrt((y ** 2).sum(1)).view(1, -1)
    return 1.0 - torch.mm(x, y.t()) / (xn + 1e-10) / (yn + 1e-10)


def _relaxed_emd(x, y):
    """appearance_loss.py:158-174: max of the two mean nearest-neighbour cosine distances."""
    d = _pairwise_cos(x, y)
    return torch.max(d.min(1)[0].mean(), d.min(0)[0].mean())


def _moment_loss(x, y):
    """appearance_loss.py:176-192: mean |mu_x - mu_y| + mean |cov_x - cov_y| (unbiased covariances), x [N,d], y [M,d]."""
    mx, my = x.mean(0, keepdim=True), y.mean(0, keepdim=True)
    xc, yc = x - mx, y - my
    cx = torch.mm(xc.t(), xc) / (x.shape[0] - 1)
    cy = torch.mm(yc.t(), yc) / (y.shape[0] - 1)
    return (mx - my).abs().mean() + (cx - cy).abs().mean()


def ot_loss_single(target_feats, gen_feats, n_samples=1000):
    """appearance_loss.py:194-210 for ONE generated image: per style layer, (sub-sampled when the map is larger than
    32x32: np.random.choice(h*w, 1000, replace=False), sorted -- the same consumption of numpy's global stream) relaxed
    EMD + moment loss between the target's and the image's feature vectors."""
    loss = 0
    for t, gfeat in zip(target_feats, gen_feats):
        c, h, w = t.shape[1], t.shape[2], t.shape[3]
        tv, gv = t.reshape(c, -1), gfeat.reshape(c, -1)
        if h > 32:
            idx = torch.as_tensor(np.sort(np.random.choice(np.arange(h * w), size=n_samples, replace=False)), device=t.device)
            tv, gv = tv[:, idx], gv[:, idx]
        tv, gv = tv.t(), gv.t()          # [N, d]
        loss = loss + _relaxed_emd(tv, gv) + _moment_loss(tv, gv)
    return loss


def _ot_layer_indices(target_feats, B, n_samples, device, np_dtype, idx_source=None):
    """The sampled positions of every style layer for a batch of B: per layer None (a map of 32 x 32 or smaller: every position)
    or an integer tensor [B, n_samples] on `device`, ascending per row.  idx_source None: drawn from numpy's global stream exactly
    as the reference's loop draws them (sample-major, layer-minor), as `np_dtype`.  Otherwise idx_source(li, B, HW, n, device)
    supplies each sampled layer's tensor and numpy's stream is not touched."""
    sampled = [t.shape[2] > 32 for t in target_feats]
    if idx_source is not None:
        out = []
        for li, t in enumerate(target_feats):
            ix = idx_source(li, B, t.shape[2] * t.shape[3], n_samples, device) if sampled[li] else None
            if ix is not None and (tuple(ix.shape) != (B, n_samples) or ix.device.type != torch.device(device).type or ix.dtype.is_floating_point):
                raise ValueError(f"ncahip.loss: idx_source returned {tuple(ix.shape)} {ix.dtype} on {ix.device} for layer {li}; "
                                 f"an integer tensor [{B}, {n_samples}] on {device} is required")
            out.append(ix)
        return out
    idx = [[None] * len(target_feats) for _ in range(B)]
    for b in range(B):                                     # the reference's draw order: sample-major, layer-minor
        for li, t in enumerate(target_feats):
            if sampled[li]:
                idx[b][li] = np.sort(np.random.choice(np.arange(t.shape[2] * t.shape[3]), size=n_samples, replace=False))
    return [torch.as_tensor(np.stack([idx[b][li] for b in range(B)]).astype(np_dtype, copy=False)).to(device) if sampled[li] else None
            for li in range(len(target_feats))]


def ot_loss_batched(target_feats, gen_feats, n_samples=1000, idx_source=None):
    """The batch mean of ot_loss_single (appearance_loss.py:212-220) without the per-sample Python loop: the sub-sampling
    indices are drawn sample by sample, layer by layer, exactly as the loop would draw them from numpy's global stream; the
    cosine-distance, nearest-neighbour and covariance products then run as batched GEMMs over all samples of a layer.

    idx_source (here and in ot_loss_fused / ot_loss_fused_all): None, or a callable (li, B, HW, n, device) -> integer tensor [B, n]
    on `device`, ascending per row, that supplies the sampled positions of layer li instead; no np.random call is then made
    (Loss(ot_index_rng="philox") passes the keyed sampler of ops.ot_sample_idx)."""
    B = gen_feats[0].shape[0]
    idx = _ot_layer_indices(target_feats, B, n_samples, target_feats[0].device, np.int64, idx_source)
    total = 0
    for li, (t, g) in enumerate(zip(target_feats, gen_feats)):
        c = t.shape[1]
        tv, gv = t.reshape(1, c, -1), g.reshape(B, c, -1)
        if idx[li] is not None:
            ix = idx[li].long()                                                                      # [B, N]
            gv = torch.gather(gv, 2, ix[:, None, :].expand(B, c, -1))
            tv = tv.expand(B, c, -1).gather(2, ix[:, None, :].expand(B, c, -1))
        else:
            tv = tv.expand(B, c, -1)
        x, y = tv.transpose(1, 2), gv.transpose(1, 2)                                               # [B, N, d]
        xn = torch.sqrt((x ** 2).sum(2))[:, :, None]
        yn = torch.sqrt((y ** 2).sum(2))[:, None, :]
        d = 1.0 - torch.bmm(x, y.transpose(1, 2)) / (xn + 1e-10) / (yn + 1e-10)
        remd = torch.maximum(d.min(2)[0].mean(1), d.min(1)[0].mean(1))                              # [B]
        mx, my = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
        xc, yc = x - mx, y - my
        n = x.shape[1]
        cx = torch.bmm(xc.transpose(1, 2), xc) / (n - 1)
        cy = torch.bmm(yc.transpose(1, 2), yc) / (n - 1)
        mom = (mx - my).abs().mean(dim=(1, 2)) + (cx - cy).abs().mean(dim=(1, 2))
        total = total + (remd + mom).sum()
    return total / B


def ot_loss_fused(target_feats, gen_feats, n_samples=1000, idx_source=None):
    """ot_loss_batched with the relaxed-EMD part on this library's kernels (csrc/nca_ot.hip): the same index draws from numpy's
    global stream in the same order (sample-major, layer-minor), one gather kernel per layer instead of expand / gather /
    transpose, and the B x N x N cosine distances reduced to their row and column minima in registers, forwards and backwards
    (the backward of a min is a gather through its argmin).  The moment term is `_moment_loss`'s arithmetic, batched, on the
    X, Y the gather kernel produced.  CUDA float32 features only (no CPU fallback); c a multiple of 4 up to 512, N <= 1024.

    The one place where the two paths differ on purpose: an all-zero generated feature vector.  In d d_ij / d y_j =
    -xh / s + <xh, y_j> y_j / (|y_j| s^2) the second term is 0 / 0 at y_j = 0; torch's autograd of sqrt at 0 turns that into NaN
    for the whole vector whenever a zero y_j sits on the winning branch, the kernel takes the term as 0 and returns the finite
    first term.  Every finite case agrees with the torch path up to summation order."""
    from .autograd import OTGather, OTRelaxedEMD
    B = gen_feats[0].shape[0]
    idx = _ot_layer_indices(target_feats, B, n_samples, gen_feats[0].device, np.int32, idx_source)
    total = 0
    for li, (t, g) in enumerate(zip(target_feats, gen_feats)):
        ix = None if idx[li] is None else idx[li].to(torch.int32)                                    # [B, N]
        x, y, xn, yn = OTGather.apply(t, g, ix)                                                      # [B, N, c]
        remd = OTRelaxedEMD.apply(x, y, xn, yn)                                                      # [B]
        mx, my = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
        xc, yc = x - mx, y - my
        n = x.shape[1]
        cx = torch.bmm(xc.transpose(1, 2), xc) / (n - 1)
        cy = torch.bmm(yc.transpose(1, 2), yc) / (n - 1)
        mom = (mx - my).abs().mean(dim=(1, 2)) + (cx - cy).abs().mean(dim=(1, 2))
        total = total + (remd + mom).sum()
    return total / B


def ot_loss_fused_all(target_feats, gen_feats, n_samples=1000, idx_source=None):
    """ot_loss_fused with the moment term on this library's kernels as well (csrc/nca_ot_moment.hip): the same index draws from
    numpy's global stream in the same order (sample-major, layer-minor); per layer the gather, the relaxed EMD and the moment term
    (means, both covariances and their difference, reduced in registers to mean |Cx - Cy| and its signs) run on library kernels,
    forwards and backwards, with one dY buffer and one scatter for both terms -- no torch matrix product anywhere.  CUDA float32
    features only (no CPU fallback); c a multiple of 4 up to 512, 2 <= N <= 1024.

    The zero-vector behaviour documented for ot_loss_fused carries over unchanged (it belongs to the relaxed EMD); the moment term
    has no singularity.  Every finite case agrees with the torch path up to summation order."""
    from .autograd import OTLayerLoss
    B = gen_feats[0].shape[0]
    idx = _ot_layer_indices(target_feats, B, n_samples, gen_feats[0].device, np.int32, idx_source)
    per_layer = []
    for li, (t, g) in enumerate(zip(target_feats, gen_feats)):
        ix = None if idx[li] is None else idx[li].to(torch.int32)                                    # [B, N]
        per_layer.append(OTLayerLoss.apply(t, g, ix))                                                # [B]
    return torch.stack(per_layer).sum() / B


_OT_IMPLS = {"batched": ot_loss_batched, "fused": ot_loss_fused, "fused_all": ot_loss_fused_all}


class Loss(nn.Module):
    def __init__(self, device, content_loss_weight=1.0, overflow_loss_weight=1.0, appearance_loss_weight=1.0,
                 appearance_loss_type="OT", target_style_image=None, feature_dtype=torch.float32, channels_last=False, ot_impl="batched",
                 slw_impl="torch", ot_index_rng="numpy", ot_index_seed=0):
        """ot_index_rng: where the OT term's sampled positions come from (layers larger than 32 x 32, 1000 positions per sample).
        'numpy' (default): np.random.choice on numpy's global stream, draw for draw as the reference.  'philox': the keyed sampler
        of ops.ot_sample_idx (csrc/nca_ot_sample.hip), one launch per sampled layer -- on the device for CUDA features, its numpy
        mirror for CPU features.  The loss then NO LONGER CONSUMES numpy's global stream: a seeded trainer run draws a different
        pool and target sequence than with 'numpy', because the draws that used to sit between the trainer's own are gone.  That is
        the point (the draws leave the host and the shared stream), and the reason it is opt-in.  The sampled positions are a
        function of the plain attributes ot_index_seed, ot_index_call (starts at 0, +1 per evaluated OT term; set it to resume a
        run) and ot_index_offset (default 0; the first sample's number, for callers that split a batch): sample b of layer li
        (index into STYLE_LAYERS) uses the row id (ot_index_call << 24) | (li << 16) | (ot_index_offset + b).  None of them is part
        of state_dict.  Works with every ot_impl; does nothing for 'Gram' / 'SlW'."""
        super().__init__()
        if ot_index_rng not in ("numpy", "philox"):
            raise ValueError(f"ncahip.loss: unknown ot_index_rng={ot_index_rng!r} ('numpy' or 'philox')")
        self.ot_index_rng = ot_index_rng
        self.ot_index_seed, self.ot_index_call, self.ot_index_offset = int(ot_index_seed), 0, 0
        if slw_impl not in _SLW_IMPLS:
            raise ValueError(f"ncahip.loss: unknown slw_impl={slw_impl!r} ('torch' or 'fused')")
        self.slw_impl = slw_impl        # 'fused': the 'SlW' term on this library's kernels (sliced_wasserstein_fused)
        if ot_impl not in _OT_IMPLS:
            raise ValueError(f"ncahip.loss: unknown ot_impl={ot_impl!r} ('batched', 'fused' or 'fused_all')")
        self.ot_impl = ot_impl          # 'fused': the relaxed-EMD part of the OT term on this library's kernels (ot_loss_fused);
                                        # 'fused_all': the moment term too (ot_loss_fused_all)
        self.device = device
        self.appearance_loss_type = appearance_loss_type
        self.appearance_loss_weight = appearance_loss_weight
        self.content_loss_weight = content_loss_weight
        self.overflow_loss_weight = overflow_loss_weight
        self.loss_weights = {}
        if overflow_loss_weight != 0:
            self.loss_weights["overflow"] = overflow_loss_weight
        if appearance_loss_weight != 0:
            assert target_style_image is not None, "Target style image required to use appearance loss"
            if appearance_loss_type not in ("OT", "Gram", "SlW"):
                raise ValueError(f"ncahip.loss: unknown appearance_loss_type={appearance_loss_type!r}")
            self.loss_weights["appearance"] = appearance_loss_weight
        if content_loss_weight != 0:
            self.loss_weights["content"] = content_loss_weight
        self.vgg = VGG16Features().to(device) if (appearance_loss_weight != 0 or content_loss_weight != 0) else None
        if self.vgg is not None and feature_dtype != torch.float32:
            self.vgg.features.to(feature_dtype)
        if self.vgg is not None and channels_last:
            self.vgg.features.to(memory_format=torch.channels_last)
        if appearance_loss_weight != 0:
            self.target_style_tensor = _to_nchw(target_style_image).to(device)
            with torch.no_grad():
                self.style_feats = self.vgg(self.target_style_tensor, STYLE_LAYERS)

    def get_overflow_loss(self, input_dict):  # loss.py:37-40
        s = input_dict["nca_state"]
        return (s - s.clamp(-1.0, 1.0)).abs().mean()

    def _ot_idx_source(self):
        """The idx_source of this evaluation of the OT term (None: numpy's global stream)."""
        if self.ot_index_rng == "numpy":
            return None
        from . import ops
        seed, call, offset = int(self.ot_index_seed), int(self.ot_index_call), int(self.ot_index_offset)

        def source(li, B, HW, n, device):
            assert 0 <= offset and offset + B <= 65536, f"ot_index_offset + B = {offset + B} exceeds the 16 bits of a row id"
            row0 = (call << 24) | (li << 16) | offset
            if torch.device(device).type == "cuda":
                return ops.ot_sample_idx(B, HW, n, seed, row0, device=device)
            return torch.from_numpy(ops.ot_sample_idx_host(B, HW, n, seed, row0))
        return source

    def ot_term(self, target_feats, gen_feats):
        """The OT appearance term (appearance_loss.py:212-220: mean over the batch) of per-layer feature lists, with this object's
        ot_impl and index source; counts the evaluation in ot_index_call."""
        acc = _OT_IMPLS[self.ot_impl](target_feats, gen_feats, idx_source=self._ot_idx_source())
        if self.ot_index_rng != "numpy":
            self.ot_index_call += 1
        return acc

    def forward(self, input_dict, return_summary=True):
        loss, log = 0, {}
        terms = {}
        if "overflow" in self.loss_weights:
            terms["overflow"] = self.get_overflow_loss(input_dict)
        if self.vgg is not None:
            gen = input_dict["generated_images"]
            need = set()
            if "appearance" in self.loss_weights:
                need |= set(STYLE_LAYERS)
            if "content" in self.loss_weights:
                need.add(CONTENT_LAYER)
            gf = self.vgg(gen, tuple(sorted(need)))
            if "appearance" in self.loss_weights:
                acc = 0
                if self.appearance_loss_type == "OT":    # appearance_loss.py:212-220: mean over the batch
                    acc = self.ot_term([self.style_feats[l] for l in STYLE_LAYERS], [gf[l] for l in STYLE_LAYERS])
                elif self.appearance_loss_type == "Gram":   # :98-106
                    for l in STYLE_LAYERS:
                        acc = acc + (_gram(self.style_feats[l]) - _gram(gf[l])).square().mean()
                else:                                       # 'SlW', :138-140: the normalised image is the first "feature" level
                    flat = lambda f: f.reshape(f.shape[0], f.shape[1], -1)
                    norm = lambda im: (im - self.vgg.mean) / self.vgg.std
                    src = [flat(norm(gen))] + [flat(gf[l]) for l in STYLE_LAYERS]
                    tgt = [flat(norm(self.target_style_tensor))] + [flat(self.style_feats[l]) for l in STYLE_LAYERS]
                    acc = sum(_SLW_IMPLS[self.slw_impl](x, y) for x, y in zip(src, tgt))
                terms["appearance"] = acc
            if "content" in self.loss_weights:
                tgt_img = input_dict["target_images"]
                if tgt_img.shape[-2:] != gen.shape[-2:]:      # content_loss.py:31-32 (torchvision resize: antialiased bilinear)
                    tgt_img = F.interpolate(tgt_img, size=gen.shape[-2:], mode="bilinear", align_corners=False, antialias=True)
                with torch.no_grad():
                    tf = self.vgg(tgt_img, (CONTENT_LAYER,))[CONTENT_LAYER]
                terms["content"] = F.mse_loss(gf[CONTENT_LAYER], tf)
        for k, v in terms.items():
            v = v * self.loss_weights[k]
            log[k] = v.detach()
            loss = loss + v
        return [loss, log if return_summary else None]
