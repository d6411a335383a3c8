"""The two-rank tests' shared parts: launch() starts a worker file under torch.distributed.run and returns its RESULT line; CASES says,
as data, what tests/dist_inference_worker.py runs, spies on, compares across the ranks and saves for each `... two ranks equal one
rank` test; inference() is the case's tools.inference call, made by the worker on every rank and by the test on one, so the two runs
a test compares cannot differ in their arguments.  Imports neither torch nor the package."""
import json
import os
import socket
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(worker, args, nproc=2, timeout=900):
    """Run tests/<worker> <args...> on nproc ranks of this box -> the parsed JSON of the last `RESULT ` line it printed."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, worker)] + [str(a) for a in args]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, p.stdout[-4000:]
    return json.loads(line[-1][7:])


# One entry per test.  Every rank runs inference(case) below once, or once per entry of `runs`, and then
#   kwargs   the keyword arguments of tools.inference on top of mvtec_inference=True, patch_localization=True; the padim and pyramid
#            tests add detector_options={"channels": ...} and pin the datamodule to imsize=(size, size) from the command line
#   spy      ("predict", paths): these attributes of the detector when predict is called, kept under the last name of the path, or
#            ("broadcast", keys): from the (state, threshold) tools.broadcast_bank returns, float(threshold) and bool(state[key])
#   gather   what the ranks exchange: one item (all_gather), a tuple of items (all_gather of their concatenation), or "object"
#            (all_gather_object of the saved dict; `equal` are the paths in it compared with torch.equal or ==, `const` the
#            paths that must hold this value on every rank)
#   file, save   the file rank 0 writes and its keys, items of the run: maps, scores (= image_scores), embeddings and what the spy saw
#   flag, result the RESULT key that says all ranks agree, and the keys after it and "world": shape, n, width, preselected
_MAPS = dict(gather="maps", file="maps_rank0.pt", save=("maps", "embeddings"), flag="maps_equal_across_ranks", result=("shape",))
_OBJECT = dict(gather="object", flag="equal_across_ranks", result=())
_PADIM = dict(gather=("maps", "image_scores", "threshold"), save=("maps", "image_scores", "embeddings", "threshold"),
              flag="equal_across_ranks")
CASES = {
    "train_bank": dict(_MAPS, kwargs=dict(bank='train')),
    "coreset": dict(_MAPS, kwargs=dict(bank='train', coreset=0.25)),
    "gde": dict(_MAPS, kwargs=dict(detector='gde')),
    "image_scores": dict(kwargs=dict(bank='train', neighbours=5),
                         runs={"max": dict(image_scores="max"), "reweighted": dict(image_scores="reweighted")},
                         gather="scores", file="scores_rank0.pt", save=("scores", "maps"), flag="equal_across_ranks", result=("n",)),
    "knn_l2": dict(_OBJECT, kwargs=dict(bank='train', image_scores='reweighted', neighbours=5, metric='euclidean', coreset=0.5),
                   spy=("predict", ("threshold", "metric", "bank_sq")),
                   file="l2_rank0.pt", save=("scores", "maps", "threshold", "bank_sq", "metric"),
                   equal=("scores", "maps", "bank_sq", "threshold"), const={"metric": "euclidean"}),
    "knn_l2_half": dict(_OBJECT, kwargs=dict(bank='train', image_scores='max', metric='euclidean', coreset=0.5, bank_dtype='float16'),
                        spy=("predict", ("threshold", "bank.dtype", "bank", "bank_sq")),
                        file="l2h_rank0.pt", save=("scores", "maps", "threshold", "dtype", "bank", "bank_sq"),
                        equal=("scores", "maps", "bank", "bank_sq", "threshold"), const={"dtype": "torch.float16"}),
    "knn_l2_int8": dict(_OBJECT, kwargs=dict(bank='train', image_scores='max', metric='euclidean', coreset=0.5, bank_dtype='int8'),
                        spy=("predict", ("threshold", "bank.dtype", "bank", "bank_sq", "quant")),
                        file="l2q_rank0.pt", save=("scores", "maps", "threshold", "dtype", "bank", "bank_sq", "quant"),
                        equal=("scores", "maps", "bank", "bank_sq", "quant", "threshold"), const={"dtype": "torch.int8"}),
    "knn_gallery": dict(_OBJECT, kwargs=dict(bank='train', image_scores='retrieval', metric='euclidean', gallery=3),
                        spy=("predict", ("threshold", "gallery", "bank_desc")),
                        file="gallery_rank0.pt", save=("scores", "maps", "threshold", "bank_desc", "gallery"),
                        equal=("scores", "maps", "bank_desc", "threshold"), const={"gallery": 3}),
    "knn_ivf": dict(_OBJECT, kwargs=dict(bank='train', image_scores='max', metric='euclidean', index='ivf', nprobe=3),
                    spy=("predict", ("threshold", "index", "ivf")),
                    file="ivf_rank0.pt", save=("scores", "maps", "threshold", "ivf", "index"),
                    equal=("scores", "maps", "threshold", "ivf.perm", "ivf.offsets", "ivf.centroids", "ivf.cent_sq"),
                    const={"index": "ivf", "ivf.nprobe": 3}),
    "padim": dict(_PADIM, kwargs=dict(detector='padim', localization='dense', bank='train', image_scores='max'),
                  spy=("broadcast", ()), file="padim_rank0.pt", result=("shape",)),
    "pyramid": dict(_PADIM, kwargs=dict(detector='padim', localization='dense', dense_features='pyramid', bank='train',
                                        image_scores='max'),
                    spy=("broadcast", ("preselected",)), file="pyramid_rank0.pt", result=("shape", "preselected", "width")),
}


def inference(tools, ck, root, case, run=None, channels=None):
    """np.random.seed(3), then tools.inference with the arguments of CASES[case] (of its run `run`, where it has several)."""
    kw = dict(CASES[case]["kwargs"], **CASES[case].get("runs", {None: {}})[run])
    if channels is not None:
        kw["detector_options"] = {"channels": channels}
    np.random.seed(3)
    return tools.inference(ck, root + "bottle/", "bottle", mvtec_inference=True, patch_localization=True, **kw)
