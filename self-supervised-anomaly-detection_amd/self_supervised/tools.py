"""Pipelines with the reference's signatures (src/self_supervised/tools.py:52-146, :204-399).

``training`` = the two-stage schedule (head only, then the whole net), ``inference`` = predict + cosine 3-NN
scoring, ``upsample`` = the fused blur+ReLU+bilinear HIP kernel, ``Evaluator`` = AUROC / F1 / AUPRO / IoU.
They drive trainer.Trainer (PyTorch Lightning is not required).  Plots (the reference's ``vis.*`` calls) are out of
scope: the histories / curves are returned or written as JSON instead."""
import json
import os
import random
import shutil
from types import SimpleNamespace

import numpy as np
import torch
from torch import Tensor

from . import metrics as mtr
from . import ops
from .constants import METRICS, EvaluationOutputContainer, ModelOutputsContainer, RegionsOutput
from .datasets import MVTecDatamodule, PretextTaskDatamodule
from . import models
from .density import position_channels
from .models import PeraNet, PositionGaussianDetector, check_bank_dtype, check_coreset, check_gallery, check_image_scores, check_index, \
    check_metric
from .trainer import MetricTracker, ModelCheckpoint, Trainer, barrier, broadcast_bank, gather_in_order, local_only, world_info


class Evaluator:
    """tools.py:52-146: scores an inference output; pixel level when ``patch_level`` (maps vs ground truths)."""

    def __init__(self, evaluation_metrics: list = [], pro_labelling: str = 'host') -> None:
        if pro_labelling not in ('host', 'device'):
            raise ValueError(f"pro_labelling is 'host' or 'device', got {pro_labelling!r}")
        self.pro_labelling = pro_labelling            # where compute_pro_gpu labels the ground truths (device maps only)
        self.evaluation_metrics = np.array(evaluation_metrics)
        self.scores = EvaluationOutputContainer()
        self.curves = {}

    def evaluate(self, output_container: ModelOutputsContainer, subject: str, outputs_dir: str, patch_level: bool = False):
        print('>>> start evaluation')
        if self.evaluation_metrics.size == 0:
            print('No metrics selected')
        bad = [m for m in self.evaluation_metrics if m not in METRICS() and m != 'ap']          # 'ap': opt-in, not a reference metric
        if bad:
            raise ValueError(f"Wrong metric(s): {bad}; correct metrics list: {METRICS()}")
        targets, scores = output_container.y_true_binary_labels, output_container.anomaly_maps
        if patch_level:
            targets = torch.flatten(output_container.ground_truths, 0, -1)
            scores = torch.flatten(scores, 0, -1)
        on_gpu = scores.is_cuda
        for m in self.evaluation_metrics:
            if m not in ('auroc', 'ap') and ((m == 'f1-score') == patch_level):
                raise ValueError(f"'{m}' not a valid metric for '{'patch' if patch_level else 'image'}-level' mode")
        if on_gpu:
            # maps still on the device (straight from tools.upsample): every sort-bound metric runs there (csrc/auroc.hip) --
            # on the host the three argsorts of a category's 6 M pixel scores take longer than training the category
            targets_dev = targets.to(scores.device)
            threshold = self._get_threshold(scores, targets_dev)         # one overridable hook for host and device maps
            if 'auroc' in self.evaluation_metrics:
                print(' pixel auroc' if patch_level else '>>> image auroc')
                self.scores.auroc = mtr.auroc_gpu(targets_dev, scores)
            if 'f1-score' in self.evaluation_metrics:
                self.scores.f1_score = mtr.compute_f1_gpu(targets_dev, scores, threshold)
            if 'aupro' in self.evaluation_metrics:
                extra = {} if self.pro_labelling == 'host' else {'labelling': self.pro_labelling}
                fprs, pros = mtr.compute_pro_gpu(output_container.anomaly_maps.squeeze(1), output_container.ground_truths.squeeze(1),
                                                 **extra)
                self.scores.aupro = mtr.compute_aupro(fprs, pros, 0.3)
                self.curves['pro'] = (fprs, pros)
            if 'iou' in self.evaluation_metrics:
                self.scores.iou = mtr.compute_iou_gpu(scores, targets_dev, threshold)
            if 'ap' in self.evaluation_metrics:
                self.scores.AP = mtr.average_precision_gpu(targets_dev, scores)
        else:
            targets, scores = targets.detach().cpu(), scores.detach().cpu()
            threshold = self._get_threshold(scores, targets)
            if 'auroc' in self.evaluation_metrics:
                print(' pixel auroc' if patch_level else '>>> image auroc')
                fpr, tpr, _ = mtr.compute_roc(targets, scores)
                self.scores.auroc = mtr.compute_auc(fpr, tpr)
                self.curves['roc'] = (fpr, tpr)
            if 'f1-score' in self.evaluation_metrics:
                self.scores.f1_score = mtr.compute_f1(targets, scores, threshold)
            if 'aupro' in self.evaluation_metrics:
                fprs, pros = mtr.compute_pro(output_container.anomaly_maps.detach().cpu().squeeze(1).numpy(),
                                             output_container.ground_truths.detach().cpu().squeeze(1).numpy())
                self.scores.aupro = mtr.compute_aupro(fprs, pros, 0.3)
                self.curves['pro'] = (fprs, pros)
            if 'iou' in self.evaluation_metrics:
                self.scores.iou = mtr.compute_iou(scores, targets, threshold)
            if 'ap' in self.evaluation_metrics:
                self.scores.AP = mtr.compute_average_precision(targets, scores)
        if outputs_dir:
            os.makedirs(outputs_dir, exist_ok=True)
            with open(os.path.join(outputs_dir, subject + ('_pixel' if patch_level else '_image') + '_scores.json'), 'w') as f:
                json.dump({k: (None if v is None else float(v)) for k, v in vars(self.scores).items()}, f)

    def _get_threshold(self, scores: Tensor, targets: Tensor):
        """F1-optimal threshold (tools.py:131-146 of the reference); device tensors take the device kernels, same value.  A subclass
        that overrides this is honoured on both routes.  (curves['roc'] is only filled for host maps: the device route returns the
        area, not the curve.)"""
        if scores.is_cuda:
            return mtr.best_f1_threshold_gpu(scores, targets)
        return mtr.best_f1_threshold(scores, targets)


def _seed_everything(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)


def training(dataset_dir: str, outputs_dir: str, subject: str, imsize: tuple = (256, 256), patch_localization: bool = False,
             patchsize: int = 32, seed: int = 0, batch_size: int = 96, projection_training_params: tuple = (10, 0.03),
             fine_tune_params: tuple = (30, 0.005), trainer_kwargs: dict = None, gpu_pipeline: bool = None) -> dict:
    """tools.py:204-306.  Returns the two metric histories (the reference plots them).
    gpu_pipeline: True = batches synthesised on the GPU from host-drawn parameter records (the sampler restates __getitem__'s draws,
    the kernels are byte-identical to the PIL path per record; batches are seeded one by one; 5.7 k img/s fp32 / 8.1 k precision 16
    at batch 96); False = the reference's input path (PretextTaskDataset.__getitem__ in 8 DataLoader workers, ~300 img/s at
    256 x 256); None (default) = SSAD_GPU_PIPELINE from the environment when set, else True: the training loop needs the GPU anyway,
    the two paths draw from the same distributions, and neither reproduces the reference's stream sample for sample (its workers
    are seeded from torch's base seed per epoch)."""
    if gpu_pipeline is None:
        gpu_pipeline = os.environ.get("SSAD_GPU_PIPELINE", "1") != "0"
    print('>>> initializing training')
    checkpoint_name = 'best_model.ckpt'
    proj_epochs, proj_lr = projection_training_params
    fine_tune_epochs, fine_tune_lr = fine_tune_params
    # under torch.distributed (one process per GPU; the reference is single-device) the filesystem side belongs to rank 0
    # and every hand-over through a file is fenced by a barrier
    rank, _ = world_info()
    if rank == 0:
        os.makedirs(outputs_dir, exist_ok=True)
        if os.path.exists(outputs_dir + 'logs/'):
            shutil.rmtree(outputs_dir + 'logs/')
    barrier()
    print('>>> setting seeds')
    _seed_everything(seed)
    print('>>> preparing datamodule')
    datamodule = PretextTaskDatamodule(subject, dataset_dir, imsize=imsize, batch_size=batch_size, seed=seed,
                                       patch_localization=patch_localization, patch_size=patchsize, gpu_pipeline=gpu_pipeline)
    datamodule.setup()
    if world_info()[1] > 1:      # SURVEY s.8e: each rank draws its own augmentations (rank-offset seed); the split above is shared
        random.seed(seed + rank)
        np.random.seed(seed + rank)
    tk = dict(trainer_kwargs or {})
    print('>>> preparing model')
    pretext_model = PeraNet(learning_rate=proj_lr, epochs=proj_epochs)
    pretext_model.freeze_net(['backbone'])
    cb = MetricTracker()
    # the reference's Trainer arguments (tools.py:260-267); trainer_kwargs may override them (e.g. precision=32)
    targs = dict(default_root_dir=outputs_dir + 'logs/', precision=16, benchmark=True, accelerator='auto', devices=1,
                 check_val_every_n_epoch=1)
    targs.update(tk)
    trainer = Trainer(callbacks=[cb], max_epochs=proj_epochs, **targs)
    print('>>> training projection head')
    trainer.fit(pretext_model, datamodule=datamodule)
    history = {'projection_train': cb.log_metrics}
    throughput = {'projection_train': list(trainer.epoch_throughput)}
    pretext_model.clear_memory_bank()
    trainer.save_checkpoint(outputs_dir + checkpoint_name, weights_only=True)     # rank 0 writes ...
    barrier()                                                                      # ... before anybody reads

    print('>>> setting up the model (fine tune whole net)')
    pretext_model = PeraNet.load_from_checkpoint(outputs_dir + checkpoint_name, learning_rate=fine_tune_lr,
                                                 epochs=fine_tune_epochs, stage='fine_tune')
    pretext_model.unfreeze()
    mc = ModelCheckpoint(dirpath=outputs_dir + 'logs/', filename='best_model_so_far', save_top_k=1, monitor="val_loss",
                         mode='min', every_n_epochs=5)
    cb = MetricTracker()
    trainer = Trainer(callbacks=[cb, mc], max_epochs=fine_tune_epochs, **targs)
    print('>>> Fine tuning')
    trainer.fit(pretext_model, datamodule=datamodule)
    trainer.save_checkpoint(outputs_dir + checkpoint_name)
    history['fine_tune'] = cb.log_metrics
    throughput['fine_tune'] = list(trainer.epoch_throughput)
    history['throughput'] = throughput          # (images, seconds) per training epoch of this rank: data feeding included
    if rank == 0:
        with open(outputs_dir + 'history.json', 'w') as f:
            json.dump(history, f)
    barrier()
    return history


def _fast_mvtec_ok(dataset):
    """The streamed predict below restates MVTecDataset.__getitem__ for the default transform only."""
    from .datasets import IMAGENET_MEAN, IMAGENET_STD, MVTecDataset
    from .tv_transforms import Compose, Normalize, ToTensor
    t = getattr(dataset, "transform", None)
    return (type(dataset) is MVTecDataset and isinstance(t, Compose) and len(t.ts) == 2 and isinstance(t.ts[0], ToTensor)
            and isinstance(t.ts[1], Normalize) and t.ts[1].mean.flatten().tolist() == torch.tensor(IMAGENET_MEAN).tolist()
            and t.ts[1].std.flatten().tolist() == torch.tensor(IMAGENET_STD).tolist()
            and os.environ.get("SSAD_FAST_PREDICT", "1") != "0")


def _decode_threads():
    """Decode threads for the streamed predict: the CPUs this process may actually use (the cgroup quota where one is set: a 1-GPU job
    on a 256-thread host is given 16), at most 16 -- Pillow's PNG inflate runs outside the GIL, so the threads scale until the quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return max(1, min(16, n, int(os.environ.get("SSAD_DECODE_THREADS", "16"))))


class _MVTecPrefetch:
    """The host half of the streamed predict, startable before the model exists: a thread pool decodes the test files (Pillow decodes
    outside the GIL) at their native size and reads the ground-truth masks exactly as ``MVTecDataset.__getitem__`` does
    (``get_ground_truth``: resize + dither to mode '1' stay Pillow's).  tools.inference starts it before it loads the checkpoint."""

    def __init__(self, dataset, indices, threads: int = None, extra_files=()):
        from concurrent.futures import ThreadPoolExecutor
        from . import gpu_io
        from .functional import get_ground_truth, get_ground_truth_filename
        self.dataset, self.indices = dataset, list(indices)
        # extra_files: images decoded and scored IN FRONT of the dataset's own (tools.inference: the training image whose embeddings
        # become the normality bank rides in the first group instead of a DataLoader pass of its own); 'good' images: all-zero masks
        self.extra = list(extra_files)
        n = len(self.extra) + len(self.indices)
        w_img, h_img = dataset.imsize
        names = self.extra + [dataset.images_filenames[i] for i in self.indices]
        self.gt8 = np.zeros((n, h_img, w_img), np.uint8)
        self.native = [None] * n
        gt_dir = dataset.dataset_dir + 'ground_truth/'

        def load(j):
            self.native[j] = gpu_io.read_native(names[j])   # decoded at its native size; the resize runs on the device (gpu_io)
            gfile = get_ground_truth_filename(names[j], gt_dir) if j >= len(self.extra) else None
            if gfile:                                        # 'good' images: Image.new(mode='1') = all zeros
                self.gt8[j] = np.asarray(get_ground_truth(gfile, dataset.imsize).convert('L'))
        self.pool = ThreadPoolExecutor(threads or _decode_threads())
        self._load, self.futs, self._next = load, [None] * n, 0
        # a sliding window of decodes ahead of the consumer (a real MVTec category is 100-170 test images of 1024 x 1024: decoding them
        # all at once would hold 0.3-0.5 GB of native-size arrays with no back-pressure from the GPU side)
        self.window = int(os.environ.get("SSAD_PREFETCH_WINDOW", "96"))
        self._submit_until(self.window)

    def _submit_until(self, end):
        end = min(end, len(self.futs))
        while self._next < end:
            self.futs[self._next] = self.pool.submit(self._load, self._next)
            self._next += 1

    def wait(self, a, b):
        self._submit_until(b + self.window)             # keep `window` images in flight beyond the group that is asked for
        for f in self.futs[a:b]:
            f.result()

    def close(self, cancel=False):
        self.pool.shutdown(wait=True, cancel_futures=cancel)


def _predict_mvtec_streamed(model: PeraNet, dataset, device, indices, group: int = 32, threads: int = None, prefetch=None):
    """``Trainer.predict`` + ``ModelOutputsContainer.from_list`` for an MVTecDataset with the default transform, as ONE stream
    instead of a DataLoader of batch size 1 (tools.py:336-347 of the reference): same values, field for field.

    * a thread pool (``_MVTecPrefetch``) decodes the files and reads the ground-truth masks;
    * ``group`` images at a time go to the device as uint8 at their NATIVE size, where Pillow's bicubic ``resize(imsize)`` (csrc/resize.hip,
      bit-exact), the 'L' -> 'RGB' replication and ToTensor + Normalize (two IEEE fp32 operations per value,
      ssad_u8hwc_to_f32chw_norm: bit-identical to the host transform) run, then ``model.forward`` -- thousands of patches per launch
      instead of 841;
    * results return to the host per group on a side stream while the next group computes; the embeddings also STAY on the device
      (second return value) for the detector, instead of making the round trip host -> device again.
    Returns (container with CPU tensors, device embeddings [n * P][D])."""
    import ctypes
    from . import _hip, gpu_io
    from .datasets import IMAGENET_MEAN, IMAGENET_STD
    from .functional import get_prediction_class
    from .converters import gt2label
    out = ModelOutputsContainer()
    pre = prefetch
    ne = len(pre.extra) if pre is not None else 0      # images in front of the dataset's own (their embeddings: out.extra_embeddings)
    n = ne + len(indices)
    if n == 0:
        if prefetch is not None:
            prefetch.close()
        return out, None
    w_img, h_img = dataset.imsize
    pre = prefetch if prefetch is not None else _MVTecPrefetch(dataset, indices, threads)
    assert pre.indices == list(indices)
    native, gt8 = pre.native, pre.gt8
    mean = (ctypes.c_float * 3)(*IMAGENET_MEAN)
    std = (ctypes.c_float * 3)(*IMAGENET_STD)
    orig = torch.empty((n, 3, h_img, w_img), dtype=torch.float32)
    xnorm = torch.empty((n, 3, h_img, w_img), dtype=torch.float32)
    emb_dev = logits_dev = emb_host = logits_host = None
    side = torch.cuda.Stream(device)
    main = torch.cuda.current_stream(device)
    lib = _hip.lib()
    pending = None                                       # (a, b, orig_dev, x_dev, event) of the group whose results are still on the device

    def drain(item):
        a, b, o_dev, x_dev, ev, p, q = item
        with torch.cuda.stream(side):
            side.wait_event(ev)
            orig[a:b].copy_(o_dev)
            xnorm[a:b].copy_(x_dev)
            emb_host[a * p:b * p].copy_(emb_dev[a * p:b * p])
            logits_host[a * q:b * q].copy_(logits_dev[a * q:b * q])
        for t in (o_dev, x_dev):
            t.record_stream(side)
    # groups of equal size, about `group` images each (97 images = 96 + the bank image: three forwards of 33 / 32 / 32, not 32 / 32 / 32
    # and a fourth one of a single image)
    ngroups = max(1, (n + group // 2) // group)
    per = -(-n // ngroups)
    try:
        with torch.no_grad():
            for a in range(0, n, per):
                b = min(n, a + per)
                pre.wait(a, b)
                img_dev = gpu_io.to_rgb_batch(native[a:b], dataset.imsize, device)
                native[a:b] = [None] * (b - a)
                o_dev = torch.empty((b - a, 3, h_img, w_img), device=device, dtype=torch.float32)
                x_dev = torch.empty_like(o_dev)
                _hip.check(lib.ssad_u8hwc_to_f32chw_norm(img_dev.data_ptr(), o_dev.data_ptr(), x_dev.data_ptr(), b - a, h_img, w_img,
                                                         mean, std, _hip.stream()))
                pred = model(x_dev)
                # rows per image: the embeddings' and the logits' (the dense mode has one row of logits per image beside its patch rows)
                p, q = pred['latent_space'].shape[0] // (b - a), pred['classifier'].shape[0] // (b - a)
                if emb_dev is None:
                    d, c = pred['latent_space'].shape[1], pred['classifier'].shape[1]
                    emb_dev = torch.empty((n * p, d), device=device, dtype=torch.float32)
                    logits_dev = torch.empty((n * q, c), device=device, dtype=torch.float32)
                    emb_host, logits_host = torch.empty((n * p, d)), torch.empty((n * q, c))
                emb_dev[a * p:b * p].copy_(pred['latent_space'])
                logits_dev[a * q:b * q].copy_(pred['classifier'])
                ev = torch.cuda.Event()
                ev.record(main)
                if pending is not None:
                    drain(pending)                          # the previous group's results travel while this group computes
                pending = (a, b, o_dev, x_dev, ev, p, q)
            drain(pending)
    except BaseException:
        pre.close(cancel=True)                           # a failing predict must not leave decode threads running until exit
        raise
    pre.close()
    side.synchronize()
    p, q = emb_dev.shape[0] // n, logits_dev.shape[0] // n
    if ne:
        # the images in front are not part of the dataset's output: their embeddings stay on the device for the caller
        out.extra_embeddings = emb_dev[:ne * p]
        orig, xnorm, gt8 = orig[ne:], xnorm[ne:], gt8[ne:]
        emb_host, logits_host, emb_dev = emb_host[ne * p:], logits_host[ne * q:], emb_dev[ne * p:]
    gts = torch.from_numpy(gt8).float().div_(255.0).unsqueeze(1)
    out.original_data, out.tensor_data, out.ground_truths = orig, xnorm, gts
    out.raw_predictions, out.embedding_vectors = logits_host, emb_host
    # (first maximum per row, as torch.max(x, 1).indices returns it -- functional.get_prediction_class -- through numpy: 1 ms
    # instead of 14 for 80 736 rows of four)
    out.y_hat = torch.from_numpy(logits_host.numpy().argmax(1))
    # predict_step labels every BATCH (of one image) from its ground truth (models.py:314-318)
    out.y_true_binary_labels = torch.tensor(gt2label(gts))
    out.y_true_multiclass_labels = torch.tensor(gt2label(gts, negative=-1, positive=model.num_classes))
    return out, emb_dev


TIMELINE = []       # SSAD_TIMELINE=1: (phase, perf_counter) marks of the last tools.inference call (tools/time_inference.py)


def _mark(name):
    if os.environ.get("SSAD_TIMELINE") == "1":
        import time
        TIMELINE.append((name, time.perf_counter()))


DETECTORS = tuple(models.DETECTORS)     # ('knn', 'gde', 'padim'): the names; models.DETECTORS maps them to the classes


def _check_detector(detector):
    if detector not in DETECTORS:
        raise ValueError(f"detector must be one of {DETECTORS}, got {detector!r}")
    return detector


BANKS = ('reference', 'train')


def _check_bank(bank, mvtec_inference=True):
    if bank not in BANKS:
        raise ValueError(f"bank must be one of {BANKS}, got {bank!r}")
    if bank == 'train' and not mvtec_inference:
        raise ValueError("bank='train' needs mvtec_inference=True: the pretext datamodule has no plain set of normal images")
    return bank


def _check_coreset(coreset, detector):
    """The coreset option of the kNN detector (models.check_coreset); the Gaussian is fitted on every row -- cheap, and a coreset
    would bias its covariance."""
    if coreset is not None and detector == 'gde':
        raise ValueError("coreset applies to detector='knn' only: the Gaussian density detector is fitted on every row")
    if coreset is not None and detector == 'padim':
        raise ValueError("coreset applies to detector='knn' only: the per-position Gaussians are fitted on every image")
    return check_coreset(coreset)


def _check_metric(metric, detector):
    """The metric option of the kNN detector (models.check_metric): 'euclidean' is PatchCore's distance between raw rows; the
    Gaussian detectors have a metric of their own (Mahalanobis)."""
    check_metric(metric)
    if metric != 'cosine' and detector != 'knn':
        raise ValueError(f"metric={metric!r} applies to detector='knn' only: detector={detector!r} scores by its Mahalanobis distance")
    return metric


def _check_gallery(gallery, detector, metric, patch_localization, bank, coreset):
    """The gallery option of the kNN detector (models.check_gallery; SPADE): Euclidean, patch level, the whole training set as the bank
    (the reference bank is ONE image: nothing to retrieve from) and no coreset."""
    if gallery is None:
        return None
    if detector != 'knn':
        raise ValueError(f"gallery applies to detector='knn' only, got detector={detector!r}")
    check_gallery(gallery, metric, coreset)
    if not patch_localization:
        raise ValueError("gallery needs patch_localization=True: it restricts the patch-level search to the retrieved images")
    if bank != 'train':
        raise ValueError("gallery needs bank='train': the reference bank is one image, there is nothing to retrieve from")
    return int(gallery)


def _check_index(index, nlist, nprobe, index_options, detector, metric, gallery):
    """The index option of the kNN detector (models.check_index; PatchCore's approximate search): 'ivf' = an inverted file over the
    bank rows, Euclidean, without a gallery; either level, localization, dense_features and bank, with or without a coreset."""
    if index != 'flat' and detector != 'knn':
        raise ValueError(f"index={index!r} applies to detector='knn' only, got detector={detector!r}")
    return check_index(index, nlist, nprobe, index_options, metric, gallery)


def _check_bank_dtype(bank_dtype, detector, metric, index, gallery, image_scores, n_neighbors=3):
    """The bank_dtype option of the kNN detector (models.check_bank_dtype; faiss' useFloat16 and QT_8bit_uniform): 'float16' = the flat
    Euclidean search with operands rounded to fp16, 'int8' = with an 8-bit scalar-quantised bank (n_neighbors 1..3); either level,
    localization, dense_features and bank, with or without a coreset."""
    if bank_dtype != 'float32' and bank_dtype in models.BANK_DTYPES and detector != 'knn':
        raise ValueError(f"bank_dtype={bank_dtype!r} applies to detector='knn' only, got detector={detector!r}")
    return check_bank_dtype(bank_dtype, metric, index, gallery, image_scores, n_neighbors)


def _check_n_neighbors(n_neighbors, detector, metric, index, gallery):
    """The n_neighbors option of the kNN detector (models.check_n_neighbors): the k of the patch score, 1..3 on every path, 4..32 on
    the flat Euclidean search; either level, localization, dense_features, bank and bank_dtype, with or without a coreset."""
    if detector != 'knn':
        if n_neighbors != 3:
            raise ValueError(f"n_neighbors={n_neighbors!r} applies to detector='knn' only, got detector={detector!r}")
        return 3
    return models.check_n_neighbors(n_neighbors, metric, index, gallery)


def _check_refine(refine, detector, bank_dtype, n_neighbors):
    """The refine option of the kNN detector (models.check_refine; faiss' IndexRefineFlat): the r nearest rows of the fp16 / int8
    search ranked again by their direct fp32 distances; r in 4..32, at least n_neighbors."""
    if refine is not None and detector != 'knn':
        raise ValueError(f"refine={refine!r} applies to detector='knn' only, got detector={detector!r}")
    return models.check_refine(refine, bank_dtype, n_neighbors)


def _check_image_scores(image_scores, neighbours, patch_localization, detector, gallery=None, index='flat'):
    """The image-score option (models.check_image_scores): patch level and the kNN detector only -- the score is taken from the patch
    scores and their nearest bank rows, which the image level and the Gaussian do not have."""
    check_image_scores(image_scores, neighbours, gallery, index)
    if image_scores is not None and not patch_localization:
        raise ValueError("image_scores needs patch_localization=True: the image level scores images already")
    if image_scores is not None and detector == 'gde':
        raise ValueError("image_scores applies to detector='knn' only: a Gaussian patch score has no nearest bank row")
    if image_scores == 'reweighted' and detector == 'padim':
        raise ValueError("image_scores='reweighted' applies to detector='knn' only: a Gaussian patch score has no nearest bank row "
                         "(detector='padim' takes image_scores='max', PaDiM's image score)")
    return image_scores


LOCALIZATIONS = ('patches', 'dense')


def _check_localization(localization, patch_localization):
    """'patches' = the reference's 841 windows per image; 'dense' = one trunk pass per image and the locally aware patch features of
    two stage maps (PeraNet.enable_dense_mode), a patch-level localisation like the first."""
    if localization not in LOCALIZATIONS:
        raise ValueError(f"localization must be one of {LOCALIZATIONS}, got {localization!r}")
    if localization == 'dense' and not patch_localization:
        raise ValueError("localization='dense' needs patch_localization=True: it is a patch-level localisation")
    return localization


PADIM_OPTIONS = ('channels', 'eps', 'seed', 'factor')


def _check_padim(detector, patch_localization, localization, bank, detector_options):
    """detector='padim' (PositionGaussianDetector) fits one Gaussian per map position over the training images: it needs
    positions that mean the same place in every image (patch_localization=True, localization='dense': one trunk pass per image) and
    more than one training image (bank='train': the reference's bank is ONE image, which gives no covariance).
    `detector_options` (channels / eps / seed / factor of the detector) belongs to 'padim' alone."""
    if detector_options is not None:
        if detector != 'padim':
            raise ValueError(f"detector_options applies to detector='padim' only, got detector={detector!r}")
        if not isinstance(detector_options, dict) or any(k not in PADIM_OPTIONS for k in detector_options):
            raise ValueError(f"detector_options must be a dict with keys among {PADIM_OPTIONS}, got {detector_options!r}")
    if detector != 'padim':
        return {}
    if not patch_localization:
        raise ValueError("detector='padim' needs patch_localization=True: it scores map positions")
    if localization != 'dense':
        raise ValueError("detector='padim' needs localization='dense': its positions come from one trunk pass per image")
    if bank != 'train':
        raise ValueError("detector='padim' needs bank='train': one training image cannot give a covariance")
    opts = dict(detector_options or {})
    PositionGaussianDetector(num_patches=1, **opts)         # the detector's own argument checks, before any file is read
    return opts


DENSE_FEATURES = ('local', 'pyramid')
PYRAMID_LAYERS = ('layer1', 'layer2', 'layer3')
PYRAMID_WIDTH = 64 + 128 + 256          # the columns of layer1 .. layer3 side by side


def _check_dense_features(dense_features, localization, patch_localization):
    """'local' = PatchCore's locally aware rows of layer2 and layer3; 'pyramid' = PaDiM's and SPADE's embedding, layer1 .. layer3 as they
    are at layer1's grid (PeraNet.enable_dense_mode(features='pyramid')): a feature construction of the dense localisation."""
    if dense_features not in DENSE_FEATURES:
        raise ValueError(f"dense_features must be one of {DENSE_FEATURES}, got {dense_features!r}")
    if dense_features == 'pyramid' and not (patch_localization and localization == 'dense'):
        raise ValueError("dense_features='pyramid' needs patch_localization=True and localization='dense': it is a feature "
                         "construction of the dense localisation")
    return dense_features


def _pyramid_columns(detector, det_kw):
    """The columns the model writes with dense_features='pyramid': PaDiM's selection, drawn once from the detector's seed (every rank
    draws the same one), or None = all of them (the kNN detectors and GDE)."""
    if detector != 'padim':
        return None
    return position_channels(PYRAMID_WIDTH, det_kw.get("channels", 96), det_kw.get("seed", 0))


def _check_options(detector, metric, localization, patch_localization, bank, mvtec_inference, coreset, image_scores, neighbours, options,
                   gallery=None, dense_features='local', index='flat', nlist=None, nprobe=8, index_options=None, bank_dtype='float32',
                   n_neighbors=3, refine=None):
    """Every option check of `inference` and `sweep`, from the arguments alone; returns the detector's class and constructor arguments."""
    _check_detector(detector)
    _check_metric(metric, detector)
    _check_localization(localization, patch_localization)
    _check_dense_features(dense_features, localization, patch_localization)
    _check_bank(bank, mvtec_inference)
    _check_coreset(coreset, detector)
    _check_gallery(gallery, detector, metric, patch_localization, bank, coreset)
    _check_index(index, nlist, nprobe, index_options, detector, metric, gallery)
    _check_image_scores(image_scores, neighbours, patch_localization, detector, gallery, index)
    _check_bank_dtype(bank_dtype, detector, metric, index, gallery, image_scores, n_neighbors)
    n_neighbors = _check_n_neighbors(n_neighbors, detector, metric, index, gallery)
    refine = _check_refine(refine, detector, bank_dtype, n_neighbors)
    det_kw = _check_padim(detector, patch_localization, localization, bank, options)
    if dense_features == 'pyramid' and detector == 'padim':
        det_kw.update(preselected=True, width=PYRAMID_WIDTH)     # the model writes the chosen columns only (_pyramid_columns)
        _pyramid_columns(detector, det_kw)                       # channels <= 448, before any file is read
    if coreset is not None:
        det_kw["coreset"] = coreset
    if metric != 'cosine':
        det_kw["metric"] = metric
    if gallery is not None:
        det_kw["gallery"] = gallery
    if index != 'flat':
        det_kw.update(index=index, nlist=nlist, nprobe=nprobe, index_options=index_options)
    if bank_dtype != 'float32':
        det_kw["bank_dtype"] = bank_dtype
    if n_neighbors != 3:
        det_kw["n_neighbors"] = n_neighbors
    if refine is not None:
        det_kw["refine"] = refine
    return models.DETECTORS[detector], det_kw


def _embed_files(model, tester, dataset, files):
    """Embeddings of `files` (per image: [patches][D], in order) through ``Trainer.predict`` over an UNSHUFFLED loader of batch size 1
    with the test dataset's transform -- the route for training images when the streamed predict is off."""
    from .datasets import MVTecDataset
    if not files:
        return []
    ds = MVTecDataset(dataset.dataset_dir, list(files), imsize=dataset.imsize, transform=dataset.transform)
    dm = MVTecDatamodule(dataset.dataset_dir, batch_size=1)
    preds = tester.predict(model, dataloaders=dm._loader(ds, False))
    return [torch.as_tensor(c.embedding_vectors).detach().cpu() for c in preds]


def _train_bank_rows(per_image, n_total, device):
    """This rank's per-image training embeddings (images rank, rank + world, ...) -> (rows [n_total * P][D] of every training image in
    file order, groups [rows]: the image index of each row).  One exchange under torch.distributed (gather_in_order); with one rank
    the rows stay where they are."""
    rank, world = world_info()
    if world > 1:
        per_image = gather_in_order([t.cpu() for t in per_image], n_total)
    if not per_image:
        raise ValueError("bank='train': the category has no training images (train/good is empty)")
    rows = torch.cat([t.to(device) for t in per_image]) if world > 1 or len(per_image) > 1 else per_image[0]
    groups = torch.repeat_interleave(torch.arange(len(per_image)), torch.tensor([int(t.shape[0]) for t in per_image]))
    return rows.contiguous(), groups


def _plan_inputs(dataset_dir, mvtec_inference, whole):
    """What `inference` reads: the datamodule, this rank's share of the test images (`mine`) and, with bank='train', of the training
    images (`my_train` of `train_files`), else the ONE training image the bank comes from (`bank_file` / `bank_item`); the decode threads."""
    # MVTec test data: file lists and decode threads start BEFORE the checkpoint is read, so that the first group of images is
    # decoded by the time the model is on the device (the datamodule draws nothing from the global generators)
    rank, world = world_info()
    datamodule = prefetch = mine = bank_file = bank_item = train_files = my_train = None
    if mvtec_inference:
        datamodule = MVTecDatamodule(dataset_dir, batch_size=1)
        datamodule.setup('predict')
        if _fast_mvtec_ok(datamodule.test_dataset):
            mine = list(range(rank, len(datamodule.test_dataset), world)) if world > 1 else list(range(len(datamodule.test_dataset)))
        if whole:
            # bank='train': every training image, round-robin over the ranks, embedded in the same stream as the test images (in
            # front of them); no generator draws -- no image is chosen
            train_files = list(datamodule.train_images_filenames)
            my_train = train_files[rank::world]
            if _fast_mvtec_ok(datamodule.test_dataset):     # (a rank without test images embeds its share through Trainer.predict)
                prefetch = _MVTecPrefetch(datamodule.test_dataset, mine, extra_files=my_train if mine else ())
        elif _fast_mvtec_ok(datamodule.test_dataset):
            # Which training image becomes the normality bank (tools.py:374-381: element [0] of a prediction over the SHUFFLED training
            # loader) is decided by two draws from torch's global generator -- the test loader's base seed, then the training loader's
            # base seed and its sampler's seed.  Nothing between here and there draws from it (the model is built on the meta device, the
            # forward pass uses no host generator), so the draws are made NOW, in the reference's order, and the image is decoded with
            # the test images and scored in their first group -- not by a DataLoader pass of its own after them (round 6: 95 ms of
            # host time per call).  Only the index is taken from the loader; the generator ends in the same state.
            try:
                state = torch.get_rng_state()
                torch.empty((), dtype=torch.int64).random_()                    # (the test loader's iterator, tools.py:336-347)
                ndm = MVTecDatamodule(dataset_dir, batch_size=1)
                ndm.num_workers = 0
                ndm.setup()
                it = iter(ndm.train_dataloader())
                first = it._next_index()                                         # the sampler's draw; no image is read
                bank_file = ndm.train_dataset.images_filenames[int(first[0])]
                bank_item = (ndm.train_dataset, int(first[0]))
                del it
            except Exception:                                                    # noqa: BLE001  (a DataLoader without these internals:
                torch.set_rng_state(state)                                       #  the draws are made later, by the loader itself)
                bank_file = None
            # (a rank without test images of its own -- more ranks than images -- scores nothing, the bank image included)
            prefetch = _MVTecPrefetch(datamodule.test_dataset, mine, extra_files=[bank_file] if (bank_file and mine) else ())
    return SimpleNamespace(rank=rank, world=world, datamodule=datamodule, prefetch=prefetch, mine=mine, bank_file=bank_file,
                           bank_item=bank_item, train_files=train_files, my_train=my_train)


def _load_model(model_input_dir, patch_localization, localization, prefetch, dense_features='local', columns=None):
    try:
        model = PeraNet.load_from_checkpoint(model_input_dir)
        _mark("checkpoint")
        model.eval()
        if patch_localization and localization == 'dense' and dense_features == 'pyramid':
            model.enable_dense_mode(PYRAMID_LAYERS, features='pyramid', columns=columns)
        elif patch_localization and localization == 'dense':
            model.enable_dense_mode()
        elif patch_localization:
            model.enable_patch_level_mode()
        tester = Trainer(accelerator='auto', devices=1)
    except BaseException:
        if prefetch is not None:               # no model, no predict: the decode threads are not left behind
            prefetch.close(cancel=True)
        raise
    return model, tester


def _predict(model, tester, datamodule, plan):
    """-> (output container, the embeddings where they stayed on the device else None, images this rank predicted)."""
    # under torch.distributed (one process per GPU) every rank scores its own round-robin share of the images; the
    # per-image containers are exchanged once at the end so that every rank returns the full output
    if plan.prefetch is not None:
        # the hot path of an evaluation: one stream through decode threads and large launches instead of a DataLoader of batch
        # size 1 (same values; _predict_mvtec_streamed).  The DataLoader iterator the reference creates here draws its base
        # seed from torch's global generator: the draw is kept, so that what follows (the shuffled loader of the normality
        # image) sees the same generator state
        if plan.bank_file is None and plan.train_files is None:
            torch.empty((), dtype=torch.int64).random_()
        model.to(tester.device).eval()
        _mark("model-on-device")
        output, emb_dev = _predict_mvtec_streamed(model, datamodule.test_dataset, tester.device, plan.mine, prefetch=plan.prefetch)
        _mark("predicted")
        return output, emb_dev, len(plan.mine)
    predictions = tester.predict(model, datamodule=datamodule, shard=plan.world > 1)
    output = ModelOutputsContainer()
    output.from_list(predictions)
    return output, None, len(predictions)


def _normality_rows(model, tester, output, plan, dataset_dir, subject, mvtec_inference):
    """-> (normality, groups): the rows the detector is fitted on, and with bank='train' the image index of every row (else None)."""
    if plan.train_files is not None:
        # the training images' embeddings: from the stream (in front of the test images) or, with the streamed predict off or no test
        # images on this rank, from Trainer.predict over an unshuffled loader -- the same rows either way
        extra = getattr(output, "extra_embeddings", None)
        if extra is not None:
            p_img = extra.shape[0] // len(plan.my_train)
            mine_train = [extra[j * p_img:(j + 1) * p_img] for j in range(len(plan.my_train))]
            del output.extra_embeddings
        else:
            mine_train = _embed_files(model, tester, plan.datamodule.test_dataset, plan.my_train)
        print(f' fitting on the whole training set ({len(plan.train_files)} images)')
        normality, groups = _train_bank_rows(mine_train, len(plan.train_files), tester.device)
        _mark("train-bank")
        return normality, groups
    if model.memory_bank.shape[0] > 1000:              # quirk Q3: the bank is capped at 1000 rows, so this never holds
        return model.memory_bank, None
    print(' not enough data in memory bank, sampling new data trom train set')
    if plan.bank_file is not None and getattr(output, "extra_embeddings", None) is not None:
        normality = output.extra_embeddings.cpu()       # the training image scored in front of the test images (_plan_inputs)
        del output.extra_embeddings
        return normality, None
    if plan.bank_item is not None:
        # the draws are made and the image is known, but it did not ride with test images (a rank that has none): score that very
        # image -- drawing again would pick another one
        ds_, i_ = plan.bank_item
        model.to(tester.device).eval()
        with torch.no_grad():
            one = model.predict_step(tuple(t.unsqueeze(0).to(tester.device) for t in ds_[i_]), 0)
        one.to_cpu()
        return one.embedding_vectors, None
    if mvtec_inference:
        normality_datamodule = MVTecDatamodule(dataset_dir, batch_size=1)
        normality_datamodule.num_workers = 0      # one deterministic image is read: not worth eight worker processes
    else:
        normality_datamodule = PretextTaskDatamodule(subject=subject, root_dir=dataset_dir, batch_size=1)
    normality_datamodule.setup()
    # the reference predicts the WHOLE training loader and keeps element [0] (tools.py:379-381); the first batch of a loader
    # does not depend on how far the loader is consumed afterwards (the shuffle permutation and the one draw for the workers'
    # base seed happen when iteration starts), so only that batch is predicted: same image, same RNG state, 1 / 209 of the work
    # (MVTec loader only: its __getitem__ draws no random numbers, so this also holds with in-process loading)
    output_normality = tester.predict(model, dataloaders=normality_datamodule.train_dataloader(),
                                      max_batches=1 if mvtec_inference else None)[0]
    output_normality.to_cpu()
    return output_normality.embedding_vectors, None


def _fit_or_receive(detector, normality, groups, plan):
    # on every rank, before anybody waits for a broadcast
    detector.check_fit_size(int(normality.shape[0]), None if groups is None else len(plan.train_files), int(normality.shape[1]))
    if plan.world > 1 and plan.rank != 0:
        # one bank for everybody: rank 0 draws the 70/30 split and fits, the others receive (state, threshold); a kNN bank carries its
        # metric, and what load_state derives from the state (bank_sq) it recomputes with the same kernel: the same bits
        state = broadcast_bank(None)
        detector.load_state(state[0])
        detector.threshold = state[1]
        return
    detector.fit(normality, **({} if groups is None else {"groups": groups}))      # (the default bank: the reference's fit call, unchanged)
    line = detector.describe_fit()
    if line:
        print(line)
    if plan.world > 1:
        broadcast_bank((detector.state(), detector.threshold))


def _score_and_gather(detector, output, emb_dev, n_pred, image_scores, neighbours, world, datamodule):
    print(' computing anomaly scores')
    scored = emb_dev if emb_dev is not None else output.embedding_vectors
    maps = detector.predict(scored)
    output.anomaly_maps = maps.cpu()
    _mark("maps")
    if image_scores is not None:
        # from the raw maps that are still on the device; travels with its image through the exchange below
        output.image_scores = detector.image_scores(scored, image_scores, neighbours, scores=maps.reshape(-1)).cpu()
        _mark("image-scores")
    if world > 1:
        per_image = gather_in_order(_split_container(output, n_pred), len(datamodule.test_dataset))
        output = ModelOutputsContainer()
        output.from_list(per_image)
    return output


def inference(model_input_dir: str, dataset_dir: str, subject: str, mvtec_inference: bool = True,
              patch_localization: bool = False, detector: str = 'knn', bank: str = 'reference',
              coreset=None, image_scores: str = None, neighbours: int = 9,
              localization: str = 'patches', detector_options: dict = None, metric: str = 'cosine',
              dense_features: str = 'local', index: str = 'flat', nlist: int = None, nprobe: int = 8,
              index_options: dict = None, bank_dtype: str = 'float32', n_neighbors: int = 3,
              refine: int = None, gallery: int = None) -> ModelOutputsContainer:
    """tools.py:310-390.  `detector`: 'knn' = the reference's cosine 3-NN (AnomalyDetector), 'gde' = the Gaussian density
    estimator of CutPaste (GaussianDensityDetector: Ledoit-Wolf Gaussian, Mahalanobis distance; needs >= 2 fit rows).
    `bank`: what the detector is fitted on.  'reference' (default) = the reference's: ONE training image drawn by a shuffled loader
    (quirks Q3 / Q4), so image-level 'gde' raises.  'train' = every image of train/good in file order (one row per image at image
    level, its patches at patch level), the 70/30 split drawn over images; MVTec data only.
    `coreset`: None (default) = the kNN bank keeps every row; a fraction in (0, 1] or an int >= 1 = a greedy k-center coreset of
    that many of the bank rows left after the split (AnomalyDetector(coreset=...)); 'knn' only.
    `image_scores`: None (default) = maps only, as the reference; 'max' / 'reweighted' = the container also carries
    `image_scores` [n_images] (test-set file order): the largest raw patch score of every image, for 'reweighted' weighted by the
    `neighbours` (2..32, default 9) bank rows around its nearest bank row (AnomalyDetector.image_scores; PatchCore eq. 6-7).  Needs
    patch_localization=True and detector='knn'; the maps are unchanged.
    `localization`: how patch_localization=True gets its rows.  'patches' (default) = the reference's 32 x 32 windows at stride 8, one
    trunk pass per window (29 x 29 maps for 256 x 256 images); 'dense' = one trunk pass per image, rows = the locally aware patch
    features of the layer2 and layer3 maps (PeraNet.enable_dense_mode: 32 x 32 maps, 384 columns); everything after the rows is the
    same code.
    detector='padim' = one Gaussian per map position (PositionGaussianDetector: PaDiM; the Mahalanobis distance to the position's
    Gaussian over `channels` randomly chosen columns); needs patch_localization=True, localization='dense' and bank='train'; takes
    image_scores='max' (PaDiM's image score) but no coreset.  `detector_options`: {'channels', 'eps', 'seed', 'factor'} of that detector
    ('padim' only).
    `metric`: 'cosine' (default) = the reference's distance; 'euclidean' = PatchCore's Euclidean distance between the raw rows
    (AnomalyDetector(metric='euclidean'): search, coreset selection and image scores all in that metric); 'knn' only.
    `gallery`: None (default) = every patch meets the whole bank; an int K >= 1 = SPADE's image-conditioned gallery
    (AnomalyDetector(gallery=K)): every test image is scored against the rows of the K training images nearest to it by the mean
    of their rows.  Needs detector='knn', metric='euclidean', patch_localization=True, bank='train' and coreset=None; either
    localization; image_scores 'max' or 'retrieval' (SPADE's image score: the mean distance to the K retrieved images).
    `dense_features`: the rows of localization='dense'.  'local' (default) = the locally aware patch features above; 'pyramid' =
    PaDiM's and SPADE's embedding: layer1, layer2 and layer3 as they are, the coarser maps replicated to layer1's grid, 448 columns
    (PeraNet.enable_dense_mode(features='pyramid'): 64 x 64 maps for 256 x 256 images).  With detector='padim' the model writes only
    the detector's `channels` columns (density.position_channels(448, channels, seed), the same draw on every rank) and the detector
    reads them as they are (PositionGaussianDetector(preselected=True)); every other detector gets all 448.
    `index`: 'flat' (default) = the exact search; 'ivf' = an inverted file over the bank rows (AnomalyDetector(index='ivf'); PatchCore's
    approximate search): `nlist` k-means cells (None: ceil(sqrt(R)) clamped to 1..4096), every patch meets the rows of its `nprobe`
    nearest cells only -- approximate for nprobe < nlist, the scores never below the exact ones; `index_options`: {'iters', 'seed',
    'train_rows'} of the k-means.  Needs detector='knn', metric='euclidean' and gallery=None; either level, localization,
    dense_features and bank; with `coreset` the index is built over the rows the coreset kept; image_scores 'max' only.
    `bank_dtype`: 'float32' (default) = the bank rows as they are; 'float16' = the flat Euclidean search with half-precision operands
    (AnomalyDetector(bank_dtype='float16'); faiss' useFloat16): bank rows and queries ARE ROUNDED TO fp16, so the distances are those
    between the rounded rows; the bank takes half the memory, on every rank and in the broadcast.  Needs detector='knn',
    metric='euclidean', index='flat' and gallery=None; either level, localization, dense_features and bank, with or without a
    coreset (selected on the fp32 rows); image_scores 'max' only.  'int8' = an 8-bit scalar-quantised bank
    (AnomalyDetector(bank_dtype='int8'); faiss' QT_8bit_uniform): one affine code over the range of the bank rows that are kept, the
    bank a quarter of the fp32 bytes, the distances THOSE BETWEEN THE CODES (plus what the clamp to the bank's range took from a
    query), within s sqrt(D) of the fp32 ones for queries inside that range (s = range / 255).  Same conditions, and n_neighbors 1..3.
    `n_neighbors`: the k of the kNN score (AnomalyDetector(n_neighbors=k); sklearn's n_neighbors, PatchCore's anomaly_scorer_num_nn,
    SPADE's kappa), default 3 as the reference: maps, threshold and the patch scores under `image_scores` are the mean distance to
    the k nearest bank rows.  1..3 on every path; 4..32 need metric='euclidean', index='flat' and gallery=None (either bank_dtype).
    'knn' only.  Not the `neighbours` above, which sizes the reweighting neighbourhood of image_scores='reweighted'.
    `refine`: None (default) = the answer of the search as it is; an int r in 4..32, at least n_neighbors, with bank_dtype 'float16' or
    'int8' (AnomalyDetector(refine=r); faiss' IndexRefineFlat) = the compressed search's r nearest rows are ranked again by their
    direct fp32 distances to the original rows, which the bank then keeps beside the compressed ones (4 D bytes per row more, on every
    rank and in the broadcast): every score is the mean of direct fp32 distances to real bank rows, equal to the exact search's
    whenever its k nearest are all in the shortlist."""
    cls, det_kw = _check_options(detector, metric, localization, patch_localization, bank, mvtec_inference, coreset, image_scores,
                                 neighbours, detector_options, gallery, dense_features, index, nlist, nprobe, index_options, bank_dtype,
                                 n_neighbors, refine)
    del TIMELINE[:]
    print('>>> initializing inference')
    plan = _plan_inputs(dataset_dir, mvtec_inference, bank == 'train')
    print('>>> preparing model')
    _mark("prefetch-started")
    columns = _pyramid_columns(detector, det_kw) if dense_features == 'pyramid' else None
    model, tester = _load_model(model_input_dir, patch_localization, localization, plan.prefetch, dense_features, columns)
    print('>>> preparing datamodule')
    if mvtec_inference:
        model.enable_mvtec_inference()
    datamodule = plan.datamodule if mvtec_inference else PretextTaskDatamodule(subject=subject, root_dir=dataset_dir, min_dataset_length=500, batch_size=1)
    print('>>> doing prediction')
    output, emb_dev, n_pred = _predict(model, tester, datamodule, plan)
    print('>>> anomaly detection phase')
    if patch_localization:
        det_kw.update(patch_level=True, batch=n_pred, num_patches=model.num_patches)
    detector = cls(**det_kw)
    normality, groups = _normality_rows(model, tester, output, plan, dataset_dir, subject, mvtec_inference)
    output.to_cpu()
    _fit_or_receive(detector, normality, groups, plan)
    _mark("bank-fitted")
    return _score_and_gather(detector, output, emb_dev, n_pred, image_scores, neighbours, plan.world, datamodule)


def _split_container(output: ModelOutputsContainer, n_images: int):
    return output.split(n_images)


def upsample(anomaly_maps: Tensor, target_size: int = 256, verbose: bool = True, method: str = 'reference', sigma: float = 4.0,
             border: str = 'symmetric'):
    """method='reference' (tools.py:394-399): relu(gaussian_blur(k=7)) then bilinear to target_size, one fused kernel.
    method='resize_blur' (opt-in): the map PatchCore and PaDiM define -- bilinear to target_size, THEN a Gaussian of `sigma` image
    pixels; border='symmetric' is scipy.ndimage.gaussian_filter's (their official code), 'reflect' torch's padding (anomalib);
    one kernel as well (ops.resize_gaussian).  `sigma` and `border` belong to 'resize_blur' alone."""
    if method not in ('reference', 'resize_blur'):
        raise ValueError(f"upsample: method is 'reference' or 'resize_blur', got {method!r}")
    if verbose:
        print('>>> upsampling')
    m = torch.as_tensor(anomaly_maps, dtype=torch.float32)
    if not m.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("tools.upsample runs on the MI355X HIP kernel only (no CPU fallback)")
        m = m.cuda()
    if method == 'resize_blur':
        return ops.resize_gaussian(m.contiguous(), target_size, sigma, border)
    return ops.blur_relu_bilinear(m.contiguous(), 7, target_size)


def defect_regions(anomaly_maps: Tensor, threshold: float, min_area: int = 1, connectivity: int = 8) -> RegionsOutput:
    """Where the defects are: thresholds the device maps ``tools.upsample`` returns (``maps >= threshold``; pass
    ``output.threshold`` or your own), splits the mask into connected regions, drops those smaller than ``min_area`` pixels and
    describes the rest (csrc/regions.hip; anomalib's pred_masks / pred_boxes / box_scores).  Masks and labels stay on the device;
    the regions' numbers come back in one copy.  Equal to scipy.ndimage.label + numpy on the host, exactly."""
    if connectivity not in (4, 8):
        raise ValueError(f"defect_regions: connectivity is 4 or 8, got {connectivity!r}")
    if not isinstance(min_area, (int, np.integer)) or isinstance(min_area, bool) or min_area < 1:
        raise ValueError(f"defect_regions: min_area is an integer >= 1, got {min_area!r}")
    if threshold is None or np.isnan(float(threshold)):
        raise ValueError("defect_regions: a threshold is required and cannot be NaN (pass output.threshold or your own)")
    maps = torch.as_tensor(anomaly_maps)
    if not ((maps.dim() == 3 or (maps.dim() == 4 and maps.shape[1] == 1)) and maps.numel() > 0 and maps.is_floating_point()):
        raise ValueError(f"defect_regions: float maps [n][1][H][W] or [n][H][W], got {tuple(maps.shape)} {maps.dtype}")
    if not maps.is_cuda:
        raise RuntimeError("tools.defect_regions runs on the MI355X HIP kernels only (no CPU fallback): pass the device maps of "
                           "tools.upsample")
    scores = (maps[:, 0] if maps.dim() == 4 else maps).detach().float().contiguous()
    n, h, w = scores.shape
    labels, _, offsets = ops.label_regions(scores, float(threshold), connectivity)
    r0 = int(offsets[n].item())
    area0 = ops.region_stats(labels, offsets, num_regions=r0)[0]
    mask, labels, counts, offsets = ops.region_filter(labels, offsets, area0 >= int(min_area))
    cnt = counts.cpu().tolist()
    r = sum(cnt)
    area, bbox, csum, peak, pos = ops.region_stats(labels, offsets, scores, num_regions=r)
    # one copy for all regions: nine int64 columns, the peak as its bit pattern
    table = torch.cat([area.long().unsqueeze(1), bbox.long(), csum, peak.view(torch.int32).long().unsqueeze(1),
                       pos.long().unsqueeze(1)], dim=1).cpu().numpy() if r else np.zeros((0, 9), dtype=np.int64)
    regions, k = [], 0
    for c in cnt:
        rows = []
        for a, x0, y0, x1, y1, sx, sy, pk, pp in table[k:k + c].tolist():
            rows.append({'box': (x0, y0, x1, y1), 'area': a, 'centroid': (sx / a, sy / a),
                         'score': float(np.array(pk, dtype=np.int64).astype(np.int32).view(np.float32)), 'peak': (pp % w, pp // w)})
        regions.append(rows)
        k += c
    return RegionsOutput(mask.unsqueeze(1), labels.unsqueeze(1), regions, float(threshold))


def image_auroc(output: ModelOutputsContainer) -> float:
    """Image AUROC of a patch-level run: the labels against `output.image_scores` (tools.inference(image_scores=...)), on the device
    when the scores are there (csrc/auroc.hip), else the host functions -- as Evaluator chooses."""
    scores = output.image_scores
    if scores is None:
        raise ValueError("image_auroc: the output carries no image_scores (tools.inference(..., image_scores='max' | 'reweighted'))")
    targets = torch.as_tensor(output.y_true_binary_labels)
    if scores.is_cuda:
        return mtr.auroc_gpu(targets.to(scores.device), scores)
    fpr, tpr, _ = mtr.compute_roc(targets.detach().cpu(), scores.detach().cpu())
    return float(mtr.compute_auc(fpr, tpr))


def _average_precision(targets, scores) -> float:
    """Average precision on the device when the scores are there (csrc/auroc.hip), else on the host -- as Evaluator chooses."""
    if scores.is_cuda:
        return mtr.average_precision_gpu(torch.as_tensor(targets).to(scores.device), scores)
    return mtr.compute_average_precision(torch.as_tensor(targets).detach().cpu(), scores.detach().cpu())


def image_ap(output: ModelOutputsContainer) -> float:
    """Image average precision of a patch-level run, beside image_auroc: the labels against `output.image_scores`."""
    scores = output.image_scores
    if scores is None:
        raise ValueError("image_ap: the output carries no image_scores (tools.inference(..., image_scores='max' | 'reweighted'))")
    return _average_precision(output.y_true_binary_labels, scores)


def gradcam_maps(model: PeraNet, images: Tensor, y_hat: Tensor, chunk: int = 64) -> Tensor:
    """Image-level localisation (src/evaluator.py:268-282 of the reference): a Grad-CAM saliency of the predicted class
    for every image predicted anomalous (y_hat != 0), an all-zero map otherwise; NaNs of constant maps become 0.
    images [N][3][H][H], y_hat [N] -> [N][1][H][H] on the model's device."""
    from .gradcam import GradCam
    cam = GradCam(model)
    dev = next(model.parameters()).device
    y_hat = torch.as_tensor(y_hat).reshape(-1).long()
    n, _, h, w = images.shape
    maps = torch.zeros((n, 1, h, w), device=dev, dtype=torch.float32)
    sel = torch.nonzero(y_hat != 0).reshape(-1)
    for i in range(0, sel.numel(), chunk):
        idx = sel[i:i + chunk]
        maps[idx.to(dev)] = cam(images[idx.to(images.device)], y_hat[idx])
    return torch.nan_to_num(maps)


def sweep(dataset_dir: str, outputs_dir: str, categories: list, imsize: tuple = (256, 256), patch_localization: bool = True,
          seed: int = 0, batch_size: int = 96, projection_training_params=(10, 0.03), fine_tune_params=(30, 0.005),
          metrics=('auroc', 'aupro', 'iou'), trainer_kwargs=None, tables_output: str = None, train: bool = True,
          detector: str = 'knn', bank: str = 'reference', coreset=None, image_scores: str = None, neighbours: int = 9,
          localization: str = 'patches', detector_options: dict = None, metric: str = 'cosine', upsample_method: str = 'reference',
          upsample_sigma: float = 4.0, dense_features: str = 'local', index: str = 'flat', nlist: int = None, nprobe: int = 8,
          index_options: dict = None, bank_dtype: str = 'float32', average_precision: bool = False, n_neighbors: int = 3,
          refine: int = None, gallery: int = None):
    """Category sweep (BASELINE configs[4]; the loop of src/evaluator.py:432-564 without its plots): per category
    training -> inference -> upsample -> Evaluator, one row of scores each plus an 'average' row, exported as csv /
    markdown when `tables_output` is given.  Categories are independent models: under torch.distributed (one process per
    GPU) rank r takes categories r, r + world, ... and the rows are exchanged once at the end -- no collective inside a
    category.  Returns the pandas DataFrame (identical on every rank).  `detector`, `bank`, `coreset`, `image_scores`,
    `neighbours`, `localization`, `detector_options`, `metric`, `gallery`, `dense_features`, `index`, `nlist`, `nprobe`, `index_options`, `bank_dtype`, `n_neighbors` and `refine` as in `inference`; with `image_scores` set, the image AUROC of the patch-level model (image_auroc) goes into one
    more table, patch_image_auroc.csv -- the reference-layout tables and the returned frame keep their columns.
    `upsample_method` and `upsample_sigma` go to the one `upsample` call ('resize_blur': PatchCore's / PaDiM's maps).
    `average_precision=True` (patch level) writes one more table in the same way, patch_ap.csv: the pixel AP of the upsampled maps
    (`pixel_ap`) and, with `image_scores` set, the image AP (`image_ap`, tools.image_ap)."""
    if upsample_method not in ('reference', 'resize_blur'):
        raise ValueError(f"sweep: upsample_method is 'reference' or 'resize_blur', got {upsample_method!r}")
    _check_options(detector, metric, localization, patch_localization, bank, True, coreset, image_scores, neighbours, detector_options,
                   gallery, dense_features, index, nlist, nprobe, index_options, bank_dtype, n_neighbors, refine)
    if average_precision and not patch_localization:
        raise ValueError("sweep: average_precision=True needs patch_localization=True (patch_ap.csv holds the pixel AP)")
    rank, world = world_info()
    mine = [c for i, c in enumerate(categories) if i % world == rank]
    rows, image_rows, ap_rows = {}, {}, {}
    score_kw = {} if image_scores is None else {"image_scores": image_scores, "neighbours": neighbours}
    if localization != 'patches':
        score_kw["localization"] = localization
    if detector_options is not None:
        score_kw["detector_options"] = detector_options
    if metric != 'cosine':
        score_kw["metric"] = metric
    if gallery is not None:
        score_kw["gallery"] = gallery
    if dense_features != 'local':
        score_kw["dense_features"] = dense_features
    if index != 'flat':
        score_kw.update(index=index, nlist=nlist, nprobe=nprobe, index_options=index_options)
    if bank_dtype != 'float32':
        score_kw["bank_dtype"] = bank_dtype
    if n_neighbors != 3:
        score_kw["n_neighbors"] = n_neighbors
    if refine is not None:
        score_kw["refine"] = refine
    for subject in mine:
        sub_out = os.path.join(outputs_dir, subject) + '/'
        data = os.path.join(dataset_dir, subject) + '/'
        with local_only():          # a category is a single-GPU job: no sharding / all-reduce with ranks on other categories
            if train:
                training(data, sub_out, subject, imsize=imsize, patch_localization=patch_localization, seed=seed,
                         batch_size=batch_size, projection_training_params=projection_training_params,
                         fine_tune_params=fine_tune_params, trainer_kwargs=trainer_kwargs)
            out = inference(sub_out + 'best_model.ckpt', data, subject, mvtec_inference=True,
                            patch_localization=patch_localization, detector=detector, bank=bank, coreset=coreset, **score_kw)
        if image_scores is not None:
            image_rows[subject] = image_auroc(out)
        if patch_localization:
            out.anomaly_maps = upsample(out.anomaly_maps, int(out.ground_truths.shape[-1]), verbose=False, method=upsample_method,
                                        sigma=upsample_sigma)      # stays on the device: the Evaluator's GPU metrics
        if average_precision:
            ap_rows[subject] = {'pixel_ap': _average_precision(out.ground_truths.reshape(-1), out.anomaly_maps.reshape(-1))}
            if image_scores is not None:
                ap_rows[subject]['image_ap'] = image_ap(out)
        ev = Evaluator(evaluation_metrics=[m for m in metrics if (m != 'f1-score') == patch_localization or m == 'auroc'])
        ev.evaluate(out, subject, sub_out, patch_level=patch_localization)
        rows[subject] = {k: v for k, v in vars(ev.scores).items() if v is not None}
    if world > 1:
        import torch.distributed as dist
        parts = [None] * world
        dist.all_gather_object(parts, rows)
        rows = {k: v for part in parts for k, v in part.items()}
        if image_scores is not None:
            dist.all_gather_object(parts, image_rows)
            image_rows = {k: v for part in parts for k, v in part.items()}
        if average_precision:
            dist.all_gather_object(parts, ap_rows)
            ap_rows = {k: v for part in parts for k, v in part.items()}
    cols = sorted({k for r in rows.values() for k in r})
    table = {c: [float(rows[s].get(c, float('nan'))) for s in categories] for c in cols}
    for c in cols:
        table[c].append(float(np.nanmean(table[c])))
    df = mtr.metrics_to_dataframe(table, list(categories) + ['average'])
    if tables_output and rank == 0:
        name = 'patch_all_scores' if patch_localization else 'image_all_scores'
        mtr.export_dataframe(df, tables_output + 'csv/', name + '.csv')
        try:
            mtr.export_dataframe(df, tables_output + 'markdown/', name + '.md', mode='markdown')
        except ImportError:
            pass
        if image_scores is not None:
            col = [float(image_rows[s]) for s in categories]
            idf = mtr.metrics_to_dataframe({'image_auroc': col + [float(np.nanmean(col))]}, list(categories) + ['average'])
            mtr.export_dataframe(idf, tables_output + 'csv/', 'patch_image_auroc.csv')
        if average_precision:
            ap_table = {}
            for c in ('pixel_ap',) + (('image_ap',) if image_scores is not None else ()):
                col = [float(ap_rows[s][c]) for s in categories]
                ap_table[c] = col + [float(np.nanmean(col))]
            adf = mtr.metrics_to_dataframe(ap_table, list(categories) + ['average'])
            mtr.export_dataframe(adf, tables_output + 'csv/', 'patch_ap.csv')
    return df
