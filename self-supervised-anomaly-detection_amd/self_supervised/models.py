"""PeraNet and AnomalyDetector with the reference's call surface, computed by HIP kernels.

Drop-in for src/self_supervised/models.py of gabry1998/Self-Supervised-Anomaly-Detection:
same constructor arguments, method names, return types and state_dict keys.  Numerics run in
libssad_hip.so (see engine.py / ops.py); there is no CPU fallback -- inputs must live on the GPU.
"""
import os
import warnings
from collections import OrderedDict

import numpy as np
import torch
from torch import Tensor, nn

from . import engine, knn_search, ops
from .constants import ModelOutputsContainer
from .converters import gt2label, multiclass2binary
from .density import GaussianDensityDetector, PositionGaussianDetector  # noqa: F401  (re-exported)
from .detectors import Detector, _take, split_indices, split_rows  # noqa: F401  (re-exported)
from .functional import get_prediction_class

try:                                    # optional: behave as a LightningModule when PL is installed
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:                       # PL is absent in the build image; trainer.py supplies the loop
    pl = None

    class _Base(nn.Module):
        def __init__(self):
            super().__init__()
            self.current_epoch = 0
            self.trainer = None
            self.hparams = {}
            self.logged = OrderedDict()

        def save_hyperparameters(self, **kw):
            self.hparams = dict(kw)

        def log_dict(self, metrics, **kw):
            for k, v in metrics.items():
                self.logged.setdefault(k, []).append(float(v))


_WARNED_RANDOM_BACKBONE = False


def _warn_random_backbone():
    global _WARNED_RANDOM_BACKBONE
    if not _WARNED_RANDOM_BACKBONE:
        _WARNED_RANDOM_BACKBONE = True
        warnings.warn("PeraNet: no ImageNet resnet18 weights found ($SSAD_RESNET18_WEIGHTS or torch hub cache "
                      "resnet18-f37072fd.pth); the backbone is RANDOMLY initialised.  The reference loads "
                      "IMAGENET1K_V1 (models.py:59): load a checkpoint / call load_backbone() before training.",
                      RuntimeWarning, stacklevel=3)


def _check_columns(columns, width):
    """`columns` of enable_dense_mode(features='pyramid'): a sorted, duplicate-free integer vector within [0, width) -> int64 tensor on
    the host.  ValueError for anything else."""
    try:
        c = torch.as_tensor(columns).detach().cpu()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"dense mode: columns must be a vector of integers, got {type(columns).__name__}") from e
    if c.dim() != 1 or c.numel() == 0 or c.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"dense mode: columns must be a non-empty vector of integers, got dtype {c.dtype}, shape {tuple(c.shape)}")
    c = c.long()
    if int(c.min()) < 0 or int(c.max()) >= width:
        raise ValueError(f"dense mode: columns must lie within [0, {width}) (the width of the stage pyramid), got {int(c.min())}.."
                         f"{int(c.max())}")
    if c.numel() > 1 and not bool((c[1:] > c[:-1]).all()):
        raise ValueError("dense mode: columns must be sorted ascending without duplicates")
    return c


class PeraNet(_Base):
    """src/self_supervised/models.py:21-341."""

    def __init__(self, learning_rate: float = 0.03, epochs: int = 30, layer_outputs: list = ['layer2', 'layer3'],
                 latent_space_layers: int = 5, latent_space_layers_base_dim: int = 512, num_classes: int = 4,
                 memory_bank_dim: int = 1000, stage='projection_train') -> None:
        super().__init__()
        if pl is not None:
            self.save_hyperparameters()
        else:
            self.save_hyperparameters(learning_rate=learning_rate, epochs=epochs, layer_outputs=layer_outputs,
                                      latent_space_layers=latent_space_layers,
                                      latent_space_layers_base_dim=latent_space_layers_base_dim,
                                      num_classes=num_classes, memory_bank_dim=memory_bank_dim, stage=stage)
        self.backbone = 'resnet18'
        self.layer_outputs = list(layer_outputs)
        dim_in = 512 + sum({'layer1': 64, 'layer2': 128, 'layer3': 256}[k] for k in self.layer_outputs)
        base = latent_space_layers_base_dim
        self.feature_extractor = engine.ResNet18Params()
        self.concatenator = nn.Sequential(nn.Linear(dim_in, base, bias=False), nn.BatchNorm1d(base))
        # (latent_space_layers-1) entries: hidden [Linear(nb)+BN+ReLU] blocks then Linear(bias)+BN (models.py:65-88)
        n_hidden = max(latent_space_layers - 1, 1) - 1
        layers = [nn.Sequential(nn.Linear(base, base, bias=False), nn.BatchNorm1d(base), nn.ReLU(inplace=True))
                  for _ in range(n_hidden)]
        layers += [nn.Linear(base, 512, bias=True), nn.BatchNorm1d(512)]
        self.latent_space = nn.Sequential(*layers)
        self.classifier = nn.Linear(512, num_classes)

        self.mvtec = False
        self.patch_level = False
        self.dense_layers = None        # enable_dense_mode: the stages whose maps become the patch features
        self.dense_features, self.dense_columns, self._dense_columns_dev = 'local', None, None
        self.num_classes = num_classes
        self.lr = learning_rate
        self.num_epochs = epochs
        self.stage = stage
        self.memory_bank_dim = memory_bank_dim
        self.memory_bank = torch.tensor([], device='cpu')
        self.batch = None
        self.num_patches = None
        # upper bound on the patches pushed through the trunk per kernel sequence; the bound actually used is derived per call
        # from the free HBM (_samples_per_pass: ~4 live layer1-sized tensors per sample, 60 % of what is free) and halves on an
        # out-of-memory error, so a smaller card, ranks sharing a device or a resident training graph pool get smaller passes
        # instead of failing.  Measured on an idle 288 GB card: 390.8 ms per 256 images at 16 384, 384.0 ms at 131 072, identical
        # results.  Every activation stays below 2^31 elements (131 072 x 16 x 16 x 64 would be exactly 2^31: hence the -1).
        self.max_samples_per_pass = 131072
        self.max_elements_per_tensor = 2 ** 31 - 1
        self.hbm_fraction_per_pass = 0.6
        self._plan = None
        self._frozen = set()
        # models.py:59 asks torchvision for IMAGENET1K_V1 (and fails loudly without it); there is no hub here, so the
        # same file is taken from $SSAD_RESNET18_WEIGHTS or torch's hub cache.  Without it the trunk keeps its random
        # init -- fine when a checkpoint / state dict is loaded next, useless for stage 1 of tools.training (frozen
        # backbone) -- so that case warns once per process (SSAD_ALLOW_RANDOM_BACKBONE=1 silences it).
        self.pretrained_backbone = False
        if self.classifier.weight.is_meta:          # load_from_checkpoint builds shapes only: the checkpoint supplies every tensor
            return
        for cand in (os.environ.get("SSAD_RESNET18_WEIGHTS"),
                     os.path.expanduser("~/.cache/torch/hub/checkpoints/resnet18-f37072fd.pth")):
            if cand and os.path.isfile(cand):
                self.load_backbone(cand)
                self.pretrained_backbone = True
                break
        if not self.pretrained_backbone and os.environ.get("SSAD_ALLOW_RANDOM_BACKBONE") != "1":
            _warn_random_backbone()

    def load_backbone(self, weights) -> None:
        """Load a torchvision ``resnet18`` state dict (or a path to one, e.g. resnet18-f37072fd.pth) into the trunk:
        what ``models.resnet18(weights="IMAGENET1K_V1")`` + ``fc = Identity`` leave behind (models.py:59-61)."""
        sd = torch.load(weights, map_location="cpu", weights_only=True) if isinstance(weights, (str, os.PathLike)) else weights
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
        own = self.feature_extractor.state_dict()
        missing = sorted(set(own) - set(sd))
        extra = sorted(set(sd) - set(own))
        if missing or extra:
            raise KeyError(f"not a resnet18 state dict: missing {missing[:4]}, unexpected {extra[:4]}")
        self.feature_extractor.load_state_dict(sd, strict=True)
        self._plan = None

    # ---- mode switches (models.py:149-172) ----
    def enable_patch_level_mode(self):
        self.patch_level = True

    def disable_patch_level_mode(self):
        self.patch_level = False

    DENSE_FEATURES = ('local', 'pyramid')

    def enable_dense_mode(self, layers=('layer2', 'layer3'), features='local', columns=None):
        """Dense feature-map localisation (opt-in; SPADE / PaDiM / PatchCore): in eval mode ``forward`` makes ONE trunk pass per image
        and returns 'latent_space' = the locally aware patch features of the two stage maps `layers` (finer first; two of layer1 ..
        layer3), one row per position of the finer map ([b * Hf * Wf][Cf + Cc], ops.local_patch_features), beside 'classifier' = the
        image-level logits of the same pass ([b][num_classes]).  Exact fp32 and eval mode only.
        features='pyramid' (opt-in): PaDiM's and SPADE's embedding instead -- two or three of layer1 .. layer3 in ascending order, the
        stage maps as they are, the coarser ones replicated to the finest grid, channels concatenated (ops.stage_pyramid_rows;
        layer1 .. layer3: 448 columns at a quarter of the image's side).  `columns` (pyramid only): a sorted, duplicate-free integer
        vector within [0, D) -- the rows then hold only those columns, in that order (PaDiM's random dimension reduction, made where
        the rows are written)."""
        if features not in self.DENSE_FEATURES:
            raise ValueError(f"dense mode: features must be one of {self.DENSE_FEATURES}, got {features!r}")
        layers = tuple(layers) if isinstance(layers, (tuple, list)) else (layers,)
        order = ('layer1', 'layer2', 'layer3')
        if features == 'local':
            if columns is not None:
                raise ValueError("dense mode: columns applies to features='pyramid' only")
            if len(layers) != 2 or any(k not in order for k in layers) or order.index(layers[0]) >= order.index(layers[1]):
                raise ValueError(f"dense mode takes two of {order}, the finer stage first, got {layers!r}")
        else:
            idx = [order.index(k) if k in order else -1 for k in layers]
            if len(layers) not in (2, 3) or min(idx) < 0 or any(a >= b for a, b in zip(idx, idx[1:])):
                raise ValueError(f"dense mode with features='pyramid' takes two or three of {order} in ascending order, got {layers!r}")
            if columns is not None:
                width = sum(c for name, _, c, _ in engine.BLOCKS if name in layers)
                columns = _check_columns(columns, width)
        self.dense_layers, self.dense_features, self.dense_columns = layers, features, columns
        self._dense_columns_dev = None

    def disable_dense_mode(self):
        self.dense_layers = None
        self.dense_features, self.dense_columns, self._dense_columns_dev = 'local', None, None

    def enable_mvtec_inference(self) -> None:
        self.mvtec = True

    def disable_mvtec_inference(self) -> None:
        self.mvtec = False

    def clear_memory_bank(self) -> None:
        self.memory_bank = torch.tensor([])

    def unfreeze_net(self, modules: list = ['backbone', 'latent_space']) -> None:
        if 'backbone' in modules:
            for p in self.feature_extractor.parameters():
                p.requires_grad = True
            self._frozen.discard('backbone')
        if 'latent_space' in modules:
            for m in (self.concatenator, self.latent_space):
                for p in m.parameters():
                    p.requires_grad = True
            self._frozen.discard('latent_space')

    def freeze_net(self, modules: list = ['backbone', 'latent_space']) -> None:
        if 'backbone' in modules:
            for p in self.feature_extractor.parameters():
                p.requires_grad = False
            self.feature_extractor.eval()
            self._frozen.add('backbone')
        if 'latent_space' in modules:
            for m in (self.concatenator, self.latent_space):
                for p in m.parameters():
                    p.requires_grad = False
                m.eval()
            self._frozen.add('latent_space')

    def unfreeze(self) -> None:          # LightningModule.unfreeze(), used at tools.py:282
        for p in self.parameters():
            p.requires_grad = True
        self._frozen.clear()
        self.train()

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location='cpu', **overrides):
        """LightningModule.load_from_checkpoint: rebuild from ``hyper_parameters`` (+ overrides, tools.py:277-281),
        load ``state_dict``, restore the memory bank.  Callable on the class or on an instance (quirk Q8)."""
        try:
            # memory-mapped: the tensors are read from the page cache when they move to the device, not copied into fresh host storage
            # first (the optimizer state of a full checkpoint is never touched at all)
            ck = torch.load(checkpoint_path, map_location=map_location, weights_only=False, mmap=True)
        except (RuntimeError, ValueError, TypeError):            # legacy (non-zipfile) checkpoints cannot be mapped
            ck = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
        hp = dict(ck.get('hyper_parameters', {}))
        hp.update(overrides)
        # every parameter and buffer comes from the checkpoint: build the module on the meta device (shapes only, no random
        # initialisation of 12.7 M weights: 0.2 s -> 0.03 s) and ADOPT the checkpoint's tensors
        with torch.device('meta'):
            model = cls(**hp)
        model.load_state_dict(ck['state_dict'], strict=True, assign=True)
        # (assign=True keeps every parameter's requires_grad flag)  Nothing may be left on the meta device: a non-persistent buffer or
        # a plain tensor attribute created in __init__ would otherwise fail at its first use, far from here
        left = [n for n, t in list(model.named_parameters()) + list(model.named_buffers()) if t.is_meta]
        if left:
            raise RuntimeError(f"load_from_checkpoint: {left} are not in the checkpoint's state_dict (still on the meta device)")
        model.on_load_checkpoint(ck)
        return model

    def on_save_checkpoint(self, checkpoint) -> None:
        checkpoint['memory_bank'] = self.memory_bank.to('cpu')

    def on_load_checkpoint(self, checkpoint) -> None:
        self.memory_bank = checkpoint['memory_bank'] if 'memory_bank' in checkpoint else torch.tensor([])

    # ---- forward (models.py:210-253) ----
    def _eval_plan(self):
        v = engine.param_version(self)
        if self._plan is None or self._plan.version != v:
            self._plan = engine.EvalPlan(self)
        return self._plan

    def _samples_per_pass(self, b, p, hv, wv, pd, device=None, held=0):
        """Images per trunk pass: the configured cap, fewer than 2^31 elements in the largest activation (the stem map: 1/4 of the
        network input's pixels x 64 channels per sample; the 32 x 32 patch path fuses stem + pool: 1/16), and what the free HBM
        holds (free = the driver's free bytes + what torch's allocator has cached but not handed out).  held: floats per sample
        that stay alive through the whole pass beside the activations (the stage maps of the dense mode)."""
        shrink = 4 if pd == 32 else 2
        act = max(1, (hv // shrink) * (wv // shrink) * 64)                       # floats of the largest activation per sample
        cap = min(self.max_samples_per_pass, self.max_elements_per_tensor // act)
        free, _ = torch.cuda.mem_get_info(device)
        free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        live = 4 if pd == 32 else 3                                              # tensors of that size alive at once (+ 25 % for the deeper stages)
        cap = min(cap, int(self.hbm_fraction_per_pass * free / (act * 4 * live * 1.25 + held * 4)))
        per_pass = max(1, cap // p)
        return -(-b // -(-b // per_pass))               # equal passes (256 images: 2 x 128 rather than 155 + 101)

    def _dense_geometry(self, x):
        """((H, W, C), ...) of the dense mode's stage maps for the batch x, finest first (two for features='local', two or three for
        'pyramid'); ValueError for what the mode does not cover -- raised from shapes and switches alone, before anything is launched."""
        if self.patch_level:
            raise ValueError("dense mode and patch-level mode are two localisations: disable one of them")
        if self.training:
            raise ValueError("dense mode is an inference mode: call model.eval() first")
        if engine.math_mode():
            raise ValueError("dense mode is exact fp32 only: unset SSAD_MATH (or set it to f32)")
        h, w = int(x.shape[-2]), int(x.shape[-1])
        if h < 64 or w < 64:
            raise ValueError(f"dense mode needs images of at least 64 x 64 pixels, got {h} x {w} (the reference's resize of smaller "
                             "inputs belongs to the window modes)")
        shapes = engine.stage_shapes(h, w)
        stages = tuple(shapes[k] for k in self.dense_layers)
        fine = stages[0]
        if fine[0] != fine[1]:
            raise ValueError(f"dense mode needs a square {self.dense_layers[0]} map (the detectors reshape scores to dim x dim), "
                             f"got {fine[0]} x {fine[1]} for images of {h} x {w}")
        return stages

    def _forward_dense(self, x, *stages):
        b, _, h, w = x.shape
        fine = stages[0]
        pyramid = self.dense_features == 'pyramid'
        p, d = fine[0] * fine[1], sum(s[2] for s in stages)
        sel_dev = None
        if pyramid and self.dense_columns is not None:
            if self._dense_columns_dev is None or self._dense_columns_dev.device != x.device:
                self._dense_columns_dev = ops.pyramid_sel(self.dense_columns, d, x.device)
            sel_dev = self._dense_columns_dev
            d = int(sel_dev.numel())
        self.batch, self.num_patches = b, p
        plan = self._eval_plan()
        pooled = torch.empty((b, self.concatenator[0].in_features), device=x.device, dtype=torch.float32)
        rows = torch.empty((b * p, d), device=x.device, dtype=torch.float32)        # allocated before the free HBM is read below
        held = sum(s[0] * s[1] * s[2] for s in stages)                                # every held stage map, floats per sample
        per_pass = self._samples_per_pass(b, 1, h, w, 0, x.device, held)
        i0 = 0
        while i0 < b:
            i1 = min(b, i0 + per_pass)
            try:
                maps = dict.fromkeys(self.dense_layers)
                engine.trunk_eval(plan, x[i0:i1], 0, 0, self.layer_outputs, pooled[i0:i1], maps)
                if pyramid:
                    ops.stage_pyramid_rows([maps[k] for k in self.dense_layers], out=rows[i0 * p:i1 * p], sel_dev=sel_dev)
                else:
                    ops.local_patch_features(maps[self.dense_layers[0]], maps[self.dense_layers[1]], rows[i0 * p:i1 * p])
            except torch.cuda.OutOfMemoryError:
                if per_pass == 1:
                    raise
                maps = None
                torch.cuda.empty_cache()
                per_pass = max(1, per_pass // 2)
                continue
            self.last_pass_samples = (i1 - i0) if i0 == 0 else self.last_pass_samples
            i0 = i1
        logits, _ = engine.head_eval(plan, pooled)
        return {'classifier': logits, 'latent_space': rows}

    def forward(self, x: Tensor) -> dict:
        dense = self._dense_geometry(x) if self.dense_layers is not None else None
        if not x.is_cuda:
            raise RuntimeError("PeraNet.forward runs on the MI355X HIP kernels only: move the batch to the GPU")
        x = x.contiguous().float()
        if dense is not None:
            return self._forward_dense(x, *dense)
        if self.training and torch.is_grad_enabled():
            from . import training
            return training.forward_train(self, x)
        b, _, h, w = x.shape
        pd, ps = (32, 8) if self.patch_level else (0, 0)
        p, hv, wv = ops.stem_geometry(h, w, pd, ps)[:3]
        if self.patch_level:
            self.batch, self.num_patches = b, p
        plan = self._eval_plan()
        dim_in = self.concatenator[0].in_features
        pooled = torch.empty((b * p, dim_in), device=x.device, dtype=torch.float32)
        per_pass = self._samples_per_pass(b, p, hv, wv, pd, x.device)
        i0 = 0
        while i0 < b:
            i1 = min(b, i0 + per_pass)
            try:
                engine.trunk_eval(plan, x[i0:i1], pd, ps, self.layer_outputs, pooled[i0 * p:i1 * p])
            except torch.cuda.OutOfMemoryError:
                if per_pass == 1:
                    raise
                torch.cuda.empty_cache()
                per_pass = max(1, per_pass // 2)           # the estimate was too generous for what else lives on the card
                continue
            self.last_pass_samples = (i1 - i0) * p if i0 == 0 else self.last_pass_samples
            i0 = i1
        logits, emb = engine.head_eval(plan, pooled)
        return {'classifier': logits, 'latent_space': emb}

    # ---- steps (models.py:256-333) ----
    def training_step(self, batch, batch_idx) -> Tensor:
        from . import training
        return training.training_step(self, batch, batch_idx)

    def on_train_epoch_end(self) -> None:
        self.memory_bank = self.memory_bank[-self.memory_bank_dim:].clone()

    def fill_memory_bank(self, embeds: Tensor, y: Tensor, y_hat: Tensor):
        mask = (y == 0) & (y_hat == 0)
        embeds = embeds[mask].detach().to('cpu')
        self.memory_bank = torch.cat([self.memory_bank, embeds])[-self.memory_bank_dim:].clone()

    def validation_step(self, batch, batch_idx) -> dict:
        from . import training
        x, y, _ = batch
        with torch.no_grad():
            was = self.training
            self.eval()
            out = self(x)
            self.train(was)
        loss, acc = training.cross_entropy_eval(out['classifier'], y)
        metrics = {"val_accuracy": acc, "val_loss": loss}
        self.log_dict(metrics, on_step=False, on_epoch=True, prog_bar=True)
        return metrics

    def predict_step(self, batch, batch_idx, dataloader_idx=0) -> ModelOutputsContainer:
        outputs = ModelOutputsContainer()
        x_prime, groundtruths, x = batch
        if self.mvtec:
            outputs.y_true_binary_labels = torch.tensor(gt2label(groundtruths))
            outputs.y_true_multiclass_labels = torch.tensor(gt2label(groundtruths, negative=-1, positive=self.num_classes))
            outputs.ground_truths = groundtruths
        else:
            outputs.y_true_binary_labels = multiclass2binary(groundtruths)
            outputs.y_true_multiclass_labels = groundtruths
        with torch.no_grad():
            predictions = self(x_prime)
        raw_predictions = predictions['classifier']
        outputs.original_data = x
        outputs.tensor_data = x_prime
        outputs.raw_predictions = raw_predictions
        outputs.embedding_vectors = predictions['latent_space']
        outputs.y_hat = get_prediction_class(raw_predictions)
        return outputs

    def configure_optimizers(self):
        from . import training
        optimizer = training.FusedSGD(self, self.lr, momentum=0.9, weight_decay=0.0005)
        scheduler = training.CosineWarmRestarts(optimizer, self.num_epochs)
        if self.stage == 'fine_tune':
            return [optimizer], [scheduler]
        return [optimizer], []


CORESET_SEED = 20230611   # seed of the coreset projection's own CPU generator
_CORESET_OMEGA = {}


def coreset_projection(D, d):
    """Omega [D][d] of the coreset selection (PatchCore's random projection): N(0, 1/d) entries drawn from a dedicated CPU
    torch.Generator seeded with CORESET_SEED, cached per (D, d).  Never draws from the global torch, numpy or `random` generators, so
    the reference's draw order (quirk Q5, the 70/30 split) does not move."""
    key = (int(D), int(d))
    if key not in _CORESET_OMEGA:
        g = torch.Generator(device="cpu").manual_seed(CORESET_SEED)
        _CORESET_OMEGA[key] = torch.randn(key, generator=g, dtype=torch.float64).div_(np.sqrt(key[1])).float()
    return _CORESET_OMEGA[key]


def check_coreset(coreset, coreset_dim=128):
    """ValueError unless `coreset` is None, a fraction in (0, 1] or an int >= 1, and `coreset_dim` None or a multiple of 4 in 4..1024."""
    if coreset is not None:
        if isinstance(coreset, (bool, np.bool_)) or not isinstance(coreset, (int, float, np.integer, np.floating)):
            raise ValueError(f"coreset must be None, a fraction in (0, 1] or an int >= 1, got {coreset!r}")
        if isinstance(coreset, (int, np.integer)):
            if coreset < 1:
                raise ValueError(f"coreset must be an int >= 1 (rows) or a fraction in (0, 1], got {coreset!r}")
        elif not 0.0 < coreset <= 1.0:
            raise ValueError(f"coreset as a fraction must lie in (0, 1], got {coreset!r}")
    if coreset_dim is not None:
        if isinstance(coreset_dim, (bool, np.bool_)) or not isinstance(coreset_dim, (int, np.integer)) \
                or not (4 <= coreset_dim <= 1024 and coreset_dim % 4 == 0):
            raise ValueError(f"coreset_dim must be None or a multiple of 4 in 4..1024, got {coreset_dim!r}")
    return coreset


IMAGE_SCORES = (None, 'max', 'reweighted', 'retrieval')


def check_image_scores(image_scores, neighbours=9, gallery=None, index='flat'):
    """ValueError unless `image_scores` is None, 'max', 'reweighted' or 'retrieval' and, for 'reweighted', `neighbours` an int in
    2..32 (one neighbour gives the weight 0 by the formula).  'retrieval' (SPADE's image score) exists with a gallery only, and
    'reweighted' without one only: the neighbourhood of the nearest bank row is taken over the whole bank.  With index='ivf' only
    'max' exists: 'reweighted' would search the whole bank again, which the index is there to avoid."""
    if image_scores not in IMAGE_SCORES:
        raise ValueError(f"image_scores must be one of {IMAGE_SCORES}, got {image_scores!r}")
    if index == 'ivf' and image_scores in ('reweighted', 'retrieval'):
        raise ValueError(f"image_scores={image_scores!r} does not go with index='ivf': 'reweighted' takes its neighbourhood over the "
                         "whole bank and 'retrieval' needs a gallery; index='ivf' takes image_scores='max'")
    if image_scores == 'retrieval' and gallery is None:
        raise ValueError("image_scores='retrieval' needs a gallery (gallery=K): it is the mean distance to the K retrieved images")
    if image_scores == 'reweighted' and gallery is not None:
        raise ValueError("image_scores='reweighted' does not go with a gallery: its neighbourhood is taken over the whole bank")
    if image_scores == 'reweighted':
        if isinstance(neighbours, (bool, np.bool_)) or not isinstance(neighbours, (int, np.integer)) or not 2 <= neighbours <= 32:
            raise ValueError(f"neighbours must be an int in 2..32 for image_scores='reweighted', got {neighbours!r}")
    return image_scores


def coreset_size(coreset, r):
    """Rows m the coreset keeps of r: ceil(f * r) for a fraction f, the int itself otherwise (m >= r: the whole bank)."""
    if isinstance(coreset, (int, np.integer)):
        return int(coreset)
    return int(np.ceil(float(coreset) * int(r)))


METRICS = ('cosine', 'euclidean')


def check_metric(metric):
    """ValueError unless `metric` is 'cosine' (the reference's distance) or 'euclidean' (PatchCore's and SPADE's)."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return metric


def check_gallery(gallery, metric='euclidean', coreset=None):
    """ValueError unless `gallery` is None or an int K >= 1 (SPADE's number of retrieved images) with metric='euclidean' (SPADE's
    metric; there is one gallery kernel) and no coreset (a coreset dissolves the image blocks the gallery is made of)."""
    if gallery is None:
        return None
    if isinstance(gallery, (bool, np.bool_)) or not isinstance(gallery, (int, np.integer)) or gallery < 1:
        raise ValueError(f"gallery must be None or an int K >= 1 (images retrieved per test image), got {gallery!r}")
    if metric != 'euclidean':
        raise ValueError(f"gallery needs metric='euclidean' (SPADE's metric; the gallery kernel is Euclidean), got metric={metric!r}")
    if coreset is not None:
        raise ValueError("gallery needs coreset=None: a coreset dissolves the image blocks a gallery is made of")
    return int(gallery)


BANK_DTYPES = ('float32', 'float16', 'int8')


def check_bank_dtype(bank_dtype, metric='euclidean', index='flat', gallery=None, image_scores=None, n_neighbors=3):
    """ValueError unless `bank_dtype` is 'float32' (default: the bank rows as they are), 'float16' (the flat Euclidean search with
    half-precision operands, csrc/knn_l2_half.hip: faiss' useFloat16) or 'int8' (the same search on an 8-bit scalar-quantised bank,
    csrc/knn_l2_int8.hip: faiss' QT_8bit_uniform) -- the latter two with metric='euclidean' (their kernels are Euclidean),
    index='flat' and gallery=None (it is the whole-bank search) and `image_scores` None or 'max' ('reweighted' takes direct fp32
    differences to bank rows, which a half or coded bank no longer has); 'int8' also with `n_neighbors` in 1..3."""
    if bank_dtype not in BANK_DTYPES:
        raise ValueError(f"bank_dtype must be one of {BANK_DTYPES}, got {bank_dtype!r}")
    if bank_dtype == 'float32':
        return bank_dtype
    if bank_dtype == 'int8':
        if metric != 'euclidean':
            raise ValueError(f"bank_dtype='int8' needs metric='euclidean' (the int8 kernel is Euclidean), got metric={metric!r}")
        if index != 'flat':
            raise ValueError(f"bank_dtype='int8' needs index='flat' (it is the search over the whole bank), got index={index!r}")
        if gallery is not None:
            raise ValueError("bank_dtype='int8' needs gallery=None: the gallery kernel reads fp32 bank rows")
        if image_scores not in (None, 'max'):
            raise ValueError(f"bank_dtype='int8' takes image_scores None or 'max', got {image_scores!r}: 'reweighted' takes direct fp32 "
                             "differences to bank rows, which the coded bank no longer holds")
        if isinstance(n_neighbors, (int, np.integer)) and not isinstance(n_neighbors, (bool, np.bool_)) and n_neighbors > 3:
            raise ValueError(f"bank_dtype='int8' supports n_neighbors in 1..3, got {n_neighbors}: 4..{N_NEIGHBORS_MAX} need bank_dtype "
                             "'float32' or 'float16' (a top-k search on codes is a follow-up)")
        return bank_dtype
    if metric != 'euclidean':
        raise ValueError(f"bank_dtype='float16' needs metric='euclidean' (the half-precision kernel is Euclidean), got metric={metric!r}")
    if index != 'flat':
        raise ValueError(f"bank_dtype='float16' needs index='flat' (it is the exact search over the whole bank), got index={index!r}")
    if gallery is not None:
        raise ValueError("bank_dtype='float16' needs gallery=None: the gallery kernel reads fp32 bank rows")
    if image_scores not in (None, 'max'):
        raise ValueError(f"bank_dtype='float16' takes image_scores None or 'max', got {image_scores!r}: 'reweighted' takes direct fp32 "
                         "differences to bank rows, which the half bank no longer holds")
    return bank_dtype


N_NEIGHBORS_MAX = 32       # ops.TOPK_MAX: the widest list of csrc/knn_topk.hip
N_NEIGHBORS_EVERYWHERE = 3  # what every search kernel selects (keep3)


def check_n_neighbors(n_neighbors, metric='cosine', index='flat', gallery=None):
    """ValueError unless `n_neighbors` is an int in 1..32 -- the k of the patch score (sklearn's n_neighbors, PatchCore's
    anomaly_scorer_num_nn) -- and, above 3, metric='euclidean', index='flat' and gallery=None: 1..3 run on every path, 4..32 on the
    flat Euclidean search only (csrc/knn_topk.hip; either bank_dtype)."""
    if isinstance(n_neighbors, (bool, np.bool_)) or not isinstance(n_neighbors, (int, np.integer)) or \
            not 1 <= n_neighbors <= N_NEIGHBORS_MAX:
        raise ValueError(f"n_neighbors must be an int in 1..{N_NEIGHBORS_MAX}, got {n_neighbors!r}")
    if n_neighbors <= N_NEIGHBORS_EVERYWHERE:
        return int(n_neighbors)
    supported = (f"n_neighbors above {N_NEIGHBORS_EVERYWHERE} is supported by the flat Euclidean search only (metric='euclidean', "
                 "index='flat', gallery=None; bank_dtype 'float32' or 'float16')")
    if metric != 'euclidean':
        raise ValueError(f"n_neighbors={n_neighbors} needs metric='euclidean', got metric={metric!r}: {supported}")
    if index != 'flat':
        raise ValueError(f"n_neighbors={n_neighbors} needs index='flat', got index={index!r}: {supported}")
    if gallery is not None:
        raise ValueError(f"n_neighbors={n_neighbors} needs gallery=None, got gallery={gallery!r}: {supported}")
    return int(n_neighbors)


REFINE_MIN, REFINE_MAX = 4, 32      # shortlist lengths: below 4 there is nothing to re-rank for k = 3, 32 is ops.RERANK_MAX


def check_refine(refine, bank_dtype='float32', n_neighbors=3):
    """ValueError unless `refine` is None (default: the search of the bank as it is) or an int r in 4..32 that is at least
    `n_neighbors`, with bank_dtype 'float16' or 'int8' (which already implies metric='euclidean', index='flat' and gallery=None):
    the compressed search's r nearest rows are ranked again by the direct fp32 distance to the original rows (faiss'
    IndexRefineFlat; csrc/knn_refine.hip)."""
    if refine is None:
        return None
    if isinstance(refine, (bool, np.bool_)) or not isinstance(refine, (int, np.integer)) or not REFINE_MIN <= refine <= REFINE_MAX:
        raise ValueError(f"refine must be None or an int in {REFINE_MIN}..{REFINE_MAX} (the length of the shortlist), got {refine!r}")
    if bank_dtype not in ('float16', 'int8'):
        raise ValueError(f"refine={refine} needs bank_dtype 'float16' or 'int8' (it ranks a compressed bank's shortlist again on the "
                         f"fp32 rows; the fp32 bank is searched exactly already), got bank_dtype={bank_dtype!r}")
    if isinstance(n_neighbors, (int, np.integer)) and not isinstance(n_neighbors, (bool, np.bool_)) and refine < n_neighbors:
        raise ValueError(f"refine={refine} must be at least n_neighbors={n_neighbors}: the k nearest are taken from the shortlist")
    return int(refine)


INDEXES = ('flat', 'ivf')
IVF_OPTIONS = ('iters', 'seed', 'train_rows')
IVF_MAX_NLIST = 4096


def check_index(index, nlist=None, nprobe=8, index_options=None, metric='euclidean', gallery=None):
    """ValueError unless `index` is 'flat' (the exact search) or 'ivf' (an inverted file over the bank rows: ops.kmeans_l2 cells,
    ops.l2_knn_ivf) with metric='euclidean' (the index kernel is Euclidean) and no gallery (a gallery already restricts the bank),
    `nlist` None or an int in 1..4096, `nprobe` an int >= 1 and `index_options` None or a dict with keys among IVF_OPTIONS.
    With 'flat' the three options must keep their defaults."""
    if index not in INDEXES:
        raise ValueError(f"index must be one of {INDEXES}, got {index!r}")
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if nlist is not None and not (is_int(nlist) and 1 <= nlist <= IVF_MAX_NLIST):
        raise ValueError(f"nlist must be None or an int in 1..{IVF_MAX_NLIST}, got {nlist!r}")
    if not (is_int(nprobe) and nprobe >= 1):
        raise ValueError(f"nprobe must be an int >= 1, got {nprobe!r}")
    if index_options is not None and (not isinstance(index_options, dict) or any(k not in IVF_OPTIONS for k in index_options)):
        raise ValueError(f"index_options must be a dict with keys among {IVF_OPTIONS}, got {index_options!r}")
    if index == 'flat':
        if nlist is not None or index_options is not None:
            raise ValueError("nlist and index_options apply to index='ivf' only")
        return index
    if metric != 'euclidean':
        raise ValueError(f"index='ivf' needs metric='euclidean' (the index kernel is Euclidean), got metric={metric!r}")
    if gallery is not None:
        raise ValueError("index='ivf' needs gallery=None: a gallery already restricts the bank of every query image")
    return index


def ivf_nlist(nlist, rows):
    """Cells of an inverted file over `rows` bank rows: `nlist` itself, or for None ceil(sqrt(rows)) clamped to 1..4096."""
    if nlist is not None:
        return int(nlist)
    return int(min(max(int(np.ceil(np.sqrt(int(rows)))), 1), IVF_MAX_NLIST))


def coreset_select(bank_n, m, coreset_dim=128):
    """Greedy k-center coreset of the bank rows bank_n [R][D] as the detector keeps them (L2-normalised with metric='cosine', raw
    with 'euclidean'; PatchCore): the selection runs on bank_n Omega
    (coreset_projection(D, coreset_dim), one MFMA GEMM) or, with coreset_dim None, on bank_n itself, starting from row 0.
    Returns (sel int64 [m'] in selection order, rad float32 [m']) on the bank's device (ops.coreset_greedy)."""
    if coreset_dim is None:
        p = bank_n
    else:
        omega_t = coreset_projection(bank_n.shape[1], coreset_dim).t().contiguous().to(bank_n.device)
        p = ops.linear_fwd(bank_n, omega_t)
    return ops.coreset_greedy(p, m, start=0)


class AnomalyDetector(Detector):
    """src/self_supervised/models.py:345-370: cosine 3-NN distance to a bank of normal embeddings.

    ``fit`` keeps the reference's unseeded 70/30 split (quirk Q5: depends on the global numpy RNG);
    the bank is L2-normalised once and kept on the GPU, ``predict`` = normalise + MFMA GEMM + top-3 mean.  The options below choose
    one of six ways to keep and search the bank; each is one class of knn_search.py, picked once by the constructor.

    `coreset` (opt-in; the reference keeps every row): None = the exact bank; a fraction f in (0, 1] or an int m >= 1 = ``fit`` keeps
    m = ceil(f R) (or m) of the R bank rows left after the split, chosen by a greedy k-center selection (coreset_select) on the
    normalised rows projected to `coreset_dim` dimensions (None: unprojected).  The bank is then those full-dimension normalised rows
    in selection order, and the threshold is scored against it.  m >= R launches nothing: the exact bank.

    `metric` (opt-in): 'cosine' (default) = the reference's distance; 'euclidean' = PatchCore's: the bank keeps the raw rows plus
    their squared norms `bank_sq`, every distance is sqrt(max(|x|^2 + |b|^2 - 2 <x, b>, 0)) (csrc/knn_l2.hip), the coreset is
    selected on the raw rows, and the embedding width must be a multiple of 32 (ValueError otherwise: there is no unfused form).

    `gallery` (opt-in; SPADE, Cohen & Hoshen 2020): None = every query meets the whole bank; an int K >= 1 = every query IMAGE is
    scored against the rows of the K' = min(K, T) bank images nearest to it only (T bank images of `num_patches` rows each).  Stage
    1: the image descriptor is the mean of an image's rows (ops.group_means -- this project's stand-in for SPADE's pooled
    last-stage feature), `bank_desc` holds the bank images', the squared distances are taken by direct differences (ops.l2_direct)
    and the K' nearest are the first columns of a stable ascending sort (equal distances to the smaller image).  Stage 2:
    ops.l2_knn_gallery (csrc/knn_gallery.hip), the Euclidean kernel on those images' row blocks.  Needs metric='euclidean',
    coreset=None, patch_level=True with num_patches, whole images everywhere, and for fit(split=True) `groups` with num_patches
    contiguous rows per image.  image_scores takes 'max' and 'retrieval' (the mean of the K' stage-1 distances), not 'reweighted'.

    `index` (opt-in; PatchCore's approximate search, faiss' IndexIVFFlat): 'flat' (default) = every query meets every bank row;
    'ivf' = an inverted file.  ``fit`` clusters the bank rows left after the split and the coreset into `nlist` cells (ops.kmeans_l2;
    None: ceil(sqrt(R)) clamped to 1..4096; `index_options` = {'iters', 'seed', 'train_rows'} of the k-means) and keeps the bank
    SORTED BY CELL: `bank[i]` is the caller's row `ivf['perm'][i]`, cell c the rows `ivf['offsets'][c] .. ivf['offsets'][c + 1] - 1`.
    A query meets the rows of the `nprobe` (clamped to nlist) cells whose centroids are nearest (ops.ivf_probes, ops.l2_knn_ivf):
    the search is APPROXIMATE for nprobe < nlist -- a score is never smaller than the exact one -- and exact, bit for bit, for
    nprobe = nlist.  The threshold goes through the same search.  ``kneighbors`` returns the caller's rows (before the sort); a
    slot the probed cells cannot fill is (+inf, -1).  Needs metric='euclidean' and gallery=None; works at both levels and with a
    coreset.  image_scores takes 'max' only: 'reweighted' and 'retrieval' raise.

    `bank_dtype` (opt-in; faiss' useFloat16 on its GPU flat index): 'float32' (default) = the bank rows as they are; 'float16' = THE
    OPERANDS ARE ROUNDED TO fp16: after the coreset selection (which runs on the fp32 rows) `bank` keeps the rows rounded by h
    (ops.rows_to_half: round to nearest even, saturating at +-65504, subnormal results flushed) as torch.float16 and `bank_sq` the
    squared norms of the rounded rows; the fp32 rows are dropped.  Queries are rounded the same way per call and every distance is
    that BETWEEN THE ROUNDED ROWS, on the fp16 matrix cores with fp32 accumulation (ops.l2h_knn_fused / l2h_knn_index) -- it differs
    from the fp32 search's by the rounding of the operands (relative 2^-11 per element).  Needs metric='euclidean', index='flat' and
    gallery=None; works at both levels and with a coreset; image_scores takes 'max' only.  'int8' = AN 8-BIT SCALAR-QUANTISED BANK
    (faiss' IndexScalarQuantizer, QT_8bit_uniform): after the coreset selection `fit` takes lo / hi, the smallest / largest element
    of the rows that are kept, and keeps `quant` = (lo, s), s = (hi - lo) / 255, `bank` = the codes rint((x - lo) / s) - 128 as
    torch.int8 -- a quarter of the fp32 bytes -- and `bank_sq` = the sums of their squares as torch.int32 (ops.int8_quantiser,
    ops.rows_to_int8); the fp32 rows are dropped.  Queries are coded the same way per call and every distance is that BETWEEN THE
    CODES, sqrt(s^2 D2 + excess) with D2 the exact integer squared code distance on the int8 matrix cores and excess what the clamp
    to [lo, hi] took from the query (ops.l2q_knn_fused / l2q_knn_index): it differs from the fp32 distance by at most s sqrt(D) for
    a query inside the bank's range and never exceeds it by more.  Same conditions as 'float16', and n_neighbors in 1..3.

    `refine` (opt-in, with bank_dtype 'float16' or 'int8'; faiss' IndexRefineFlat): None (default) = the compressed search's answer;
    an int r in 4..32, at least n_neighbors = the compressed search returns its r' = min(r, R) nearest rows as a SHORTLIST
    (ops.l2h_topk_index / l2q_topk_index; the k <= 3 index kernels for r' <= 3) and the score and ``kneighbors`` are taken from the
    direct fp32 distances sum (x - b)^2 of the query to those rows of `bank_f32`, the rows before rounding or coding, kept beside
    the compressed bank (4 D bytes per row more) -- ops.l2_rerank_mean / l2_rerank_index, csrc/knn_refine.hip.  Every distance
    returned is the direct fp32 distance to a real bank row, so a refined score is never below the exact search's (up to the direct
    form's rounding); it EQUALS the exact k nearest whenever they all are in the shortlist, and always when R <= r.  It does not
    promise the fp32 flat kernel's bits: that kernel uses the expanded form |x|^2 + |b|^2 - 2 <x, b>, the direct form is the more
    accurate of the two.  ``kneighbors`` takes k <= r'.  A state carries `refine` and `bank_f32`.

    `n_neighbors` (default 3, the reference's; sklearn's n_neighbors, PatchCore's anomaly_scorer_num_nn, SPADE's kappa): the k of the
    score -- the mean distance to the k nearest bank rows -- kept as `self.k` and read by ``predict``, the threshold of ``fit``, the
    patch scores inside ``image_scores`` and the default of ``kneighbors``.  1..3 run on every path with the kernels those paths
    have.  4..32 need metric='euclidean', index='flat' and gallery=None (either bank_dtype; csrc/knn_topk.hip, ops.l2_topk_mean /
    l2h_topk_mean): a pair's distance keeps the bits of the k <= 3 search, so the first three neighbours are those of n_neighbors=3.
    Cosine, gallery and IVF searches for k > 3 are a follow-up.  A bank of fewer rows than n_neighbors raises.  Not to be confused
    with the `neighbours` of ``image_scores``: that is the b of PatchCore's eq. 6-7, the size of the reweighting neighbourhood."""

    refine = None       # the shortlist length of a refined detector; an instance attribute only where the option is set

    def __init__(self, patch_level: bool = False, batch: int = None, num_patches: int = None, coreset=None,
                 coreset_dim: int = 128, metric: str = 'cosine', index: str = 'flat', nlist: int = None, nprobe: int = 8,
                 index_options: dict = None, bank_dtype: str = 'float32', n_neighbors: int = 3, refine: int = None,
                 gallery: int = None) -> None:
        super().__init__(patch_level, batch, num_patches)
        self.bank = None
        self.bank_sq = None             # metric='euclidean': squared norms of the bank rows (ops.row_sqnorms)
        self.metric = check_metric(metric)
        self.coreset = check_coreset(coreset, coreset_dim)
        self.coreset_dim = coreset_dim
        self.coreset_rows = None        # after fit with a coreset: (sel, rad) -- sel indexes the bank rows after the split
        self.coreset_counts = None      # after fit with a coreset: (rows kept, rows after the split)
        self.gallery = check_gallery(gallery, self.metric, self.coreset)
        self.bank_desc = None           # gallery: descriptors of the bank images (ops.group_means)
        if self.gallery is not None:
            if not patch_level or not num_patches or int(num_patches) < 1:
                raise ValueError("gallery needs a patch-level detector (patch_level=True with num_patches): its bank is made of images")
            self.patches = int(num_patches)
        self.index = check_index(index, nlist, nprobe, index_options, self.metric, self.gallery)
        self.nlist = None if nlist is None else int(nlist)
        self.nprobe = int(nprobe)
        self.index_options = dict(index_options or {})
        self.ivf = None                 # index='ivf' after fit: perm, offsets, centroids, cent_sq, nlist, nprobe (bank: sorted by cell)
        self.bank_dtype = check_bank_dtype(bank_dtype, self.metric, self.index, self.gallery, None, n_neighbors)
        self.k = check_n_neighbors(n_neighbors, self.metric, self.index, self.gallery)      # the one place n_neighbors is kept
        if self.bank_dtype == 'int8':
            self.quant = None           # after fit: (lo, s) of the bank's 8-bit code (ops.int8_quantiser)
        # how the bank is kept and searched: everything below delegates to it (knn_search.py); the data stays in the attributes above
        if check_refine(refine, self.bank_dtype, self.k) is None:
            self._search = knn_search.choose(self.metric, self.index, self.gallery, self.bank_dtype)
        else:                           # the default detector carries nothing of the option (`refine` is then the class's None)
            self.refine = int(refine)
            self.bank_f32 = None        # after fit: the fp32 rows of the compressed bank, what the shortlist is ranked on again
            self._search = knn_search.choose(self.metric, self.index, self.gallery, self.bank_dtype, self.refine)

    @property
    def n_neighbors(self) -> int:
        """The k of the score, as the constructor took it: `self.k` is where it is kept (the reference's attribute)."""
        return self.k

    def _whole_images(self, what, rows: int) -> int:
        if rows < 1 or rows % self.patches:
            raise ValueError(f"{what}: with a gallery, {rows} rows are not whole images of {self.patches} patches")
        return rows // self.patches

    def _check_fit(self, emb, split, groups):
        if self.gallery is None:
            return groups
        n = int(emb.shape[0])
        self._whole_images("fit", n)
        if groups is None:
            if split:
                raise ValueError("fit: with a gallery, fit(split=True) needs `groups` (the split is drawn over images)")
            return None
        g = np.asarray(torch.as_tensor(groups).cpu()).reshape(-1).astype(np.int64)
        if g.shape[0] != n:
            raise ValueError(f"groups has {g.shape[0]} entries for {n} rows")
        blocks = g.reshape(-1, self.patches)
        if not (blocks == blocks[:, :1]).all() or np.unique(blocks[:, 0]).shape[0] != blocks.shape[0]:
            raise ValueError(f"fit: with a gallery, every image must have exactly num_patches = {self.patches} contiguous rows")
        return groups

    def _after_bank(self, train) -> None:
        if self.coreset is not None:
            r = int(self.bank.shape[0])
            m = coreset_size(self.coreset, r)
            if m < r:
                rows = self._search.coreset_rows(self, train)       # fp32: the bank, or `train` again where the bank is fp16 / int8
                sel, rad = coreset_select(rows, m, self.coreset_dim)
                self._search.keep(self, sel, rows)
                self.coreset_rows = (sel, rad)
            self.coreset_counts = (int(self.bank.shape[0]), r)
        self._search.finish(self)

    def describe_fit(self):
        lines = [] if self.coreset_counts is None else [f' coreset: {self.coreset_counts[0]} of {self.coreset_counts[1]} rows']
        if self.ivf is not None:
            sizes = (self.ivf["offsets"][1:] - self.ivf["offsets"][:-1]).cpu().numpy()
            lines.append(f' ivf index: nlist {self.ivf["nlist"]}, nprobe {self.ivf["nprobe"]}, cells of {int(sizes.min())} / '
                         f'{int(np.median(sizes))} / {int(sizes.max())} rows (smallest / median / largest), {int((sizes == 0).sum())} empty')
        return '\n'.join(lines) if lines else None

    def fit_bank(self, bank: Tensor) -> None:
        self.ivf = None                 # the rows as given: an index is built by fit (_after_bank) or arrives with load_state
        self._search.store(self, bank)

    def state(self):
        """What another rank needs to score like this detector (tools.inference under torch.distributed): the metric and the bank
        rows as they are kept, on the host.  `bank_sq` does not travel: load_state recomputes it with the same kernel.  With
        bank_dtype 'float16' or 'int8' the state names it (`bank_dtype`) and `bank` holds the halves or the codes; 'int8' also
        carries `bank_sq`, `lo` and `s`.  With a gallery the state names it (`gallery`: K); `bank_desc` is recomputed like `bank_sq`.
        With index='ivf' `bank` is the bank sorted by cell and the state also carries `perm`, `offsets`, `centroids`, `nlist` and
        `nprobe`.  `n_neighbors` travels unless it is 3."""
        return self._search.state(self)

    def load_state(self, state) -> None:
        if state["metric"] != self.metric:
            raise ValueError(f"load_state: the bank was fitted with metric={state['metric']!r}, this detector has {self.metric!r}")
        if state.get("gallery") != self.gallery:
            raise ValueError(f"load_state: the bank was fitted with gallery={state.get('gallery')!r}, this detector has {self.gallery!r}")
        if state.get("bank_dtype", 'float32') != self.bank_dtype:
            raise ValueError(f"load_state: the bank was fitted with bank_dtype={state.get('bank_dtype', 'float32')!r}, this detector has "
                             f"{self.bank_dtype!r}")
        if state.get("n_neighbors", 3) != self.n_neighbors:
            raise ValueError(f"load_state: the bank was fitted with n_neighbors={state.get('n_neighbors', 3)!r}, this detector has "
                             f"{self.n_neighbors!r}")
        if state.get("refine") != self.refine:
            raise ValueError(f"load_state: the bank was fitted with refine={state.get('refine')!r}, this detector has {self.refine!r}")
        if ("nlist" in state) != (self.index == 'ivf'):
            raise ValueError(f"load_state: the bank was fitted with index={'ivf' if 'nlist' in state else 'flat'!r}, this detector has "
                             f"{self.index!r}")
        self.ivf = None
        self._search.load(self, state)

    def retrieve(self, x):
        """Stage 1 of the gallery for the whole query images x [Q * num_patches][D] (on the device): (gallery int32 [Q][K'],
        d2 float32 [Q][K']), the K' = min(K, T) bank images nearest to each query image by the squared distance between the image
        descriptors, nearest first, equal distances to the smaller image, and those squared distances."""
        return self._search.retrieve(self, x)

    def _scores(self, x):
        return self._search.scores(self, x)

    def kneighbors(self, x: Tensor, k: int = None):
        """sklearn's NearestNeighbors.kneighbors (what the reference's detector wraps) on the fitted bank: (dist [N][k] float32,
        idx [N][k] int64), the k (default self.k; 1..32 on the flat Euclidean paths, 1..3 elsewhere) nearest bank rows of every row of x by the detector's metric, nearest first, equal
        distances to the smaller row.  idx indexes self.bank (after the split and the coreset).  Works at both levels.  With a gallery
        x holds whole images and the neighbours are taken among the rows of each image's gallery (idx still indexes self.bank).
        With index='ivf' the neighbours are taken among the rows of the probed cells and idx holds the caller's rows, as index='flat'
        numbers them (self.bank[i] is row self.ivf['perm'][i]); a slot the cells cannot fill is (+inf, -1)."""
        if self.bank is None:
            raise ValueError("kneighbors: the detector has no bank (fit or fit_bank first)")
        x = self._dev(x)
        if x.shape[1] % 32:
            raise ValueError(f"kneighbors: the index kernel needs an embedding width that is a multiple of 32, got {x.shape[1]}")
        dist, idx = self._search.kneighbors(self, x, self.k if k is None else int(k))
        return dist, idx.long()

    def image_scores(self, x: Tensor, mode: str = 'max', neighbours: int = 9, scores: Tensor = None) -> Tensor:
        """Detector.image_scores; with a gallery also mode='retrieval', SPADE's image score: the mean of the K' stage-1 distances
        sqrt(d2) between the image's descriptor and those of its retrieved bank images."""
        if mode == 'retrieval':
            self._check_image_scores(mode, neighbours)
            _, d2 = self.retrieve(self._dev(x))
            return torch.sqrt(d2).mean(1)
        return super().image_scores(x, mode, neighbours, scores)

    def _check_image_scores(self, mode, neighbours) -> None:
        check_image_scores(mode, neighbours, self.gallery, self.index)
        check_bank_dtype(self.bank_dtype, self.metric, self.index, self.gallery, mode, self.k)
        if not self.patch_level or not self.dim:
            raise ValueError("image_scores needs a patch-level detector (patch_level=True with num_patches)")
        if self.bank is None:
            raise ValueError("image_scores: the detector has no bank (fit or fit_bank first)")

    def _image_patches(self, rows: int) -> int:
        if rows % self.dim ** 2:
            raise ValueError(f"image_scores: {rows} rows are not whole images of {self.dim ** 2} patches")
        return self.dim ** 2

    def _reweight(self, xs, smax, neighbours):
        """image_scores(mode='reweighted') (PatchCore eq. 6-7 with the detector's metric): w s_{p*}, w = 1 - exp(d(x_{p*}, m*)) /
        sum_{r in N} exp(d(x_{p*}, r)), m* the nearest bank row of x_{p*} (`xs`), N the min(neighbours, R) bank rows nearest to B_{m*}."""
        return self._search.reweight(self, xs, smax, neighbours)


DETECTORS = {'knn': AnomalyDetector, 'gde': GaussianDensityDetector, 'padim': PositionGaussianDetector}     # tools.inference(detector=...)
