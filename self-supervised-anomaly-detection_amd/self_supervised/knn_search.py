"""How ``models.AnomalyDetector`` keeps and searches its bank: one class per kind of bank, each holding everything that is its own --
how ``fit_bank`` stores the rows, how a coreset selection is kept, the patch scores and the k nearest neighbours, what travels in a
``state()`` and how ``load_state`` restores it, and the ``image_scores`` modes beyond 'max'.

The objects hold no data.  Every method takes the detector and reads and writes its plain attributes (`bank`, `bank_sq`, `bank_desc`,
`quant`, `ivf`, `k`, ...), so ``choose`` hands out one shared object per kind.  Device ops are looked up as ``ops.name`` when they are
called and the device is reached through the detector's ``_dev``.  Options are validated by the ``check_*`` functions of models.py
before a path is chosen: nothing here refuses a combination of them."""
import torch

from . import ops


def _state(det, **extras):
    state = {"metric": det.metric, "bank": det.bank.cpu(), **extras}
    if det.k != 3:
        state["n_neighbors"] = det.k        # absent = 3: states written before the option still load
    return state


class SearchPath:
    """What the paths share.  A subclass supplies ``store``, ``scores`` and ``kneighbors``."""

    def coreset_rows(self, det, train):
        """The fp32 rows a coreset is selected on: the bank where it holds them, else the training rows of ``fit`` once more."""
        return det.bank if det.bank.dtype == torch.float32 else det._dev(train)

    def keep(self, det, sel, rows) -> None:
        """Keeps the rows `sel` of the bank, in that order (`rows`: what ``coreset_rows`` returned)."""
        det.bank = det.bank.index_select(0, sel).contiguous()

    def finish(self, det) -> None:
        """The end of ``fit``'s bank: after the coreset, before the threshold."""

    def state(self, det):
        return _state(det)

    def load(self, det, state) -> None:
        det.bank = det._dev(state["bank"])

    def retrieve(self, det, x):
        raise ValueError("retrieve: the detector has no gallery (AnomalyDetector(gallery=K))")


class Cosine(SearchPath):
    """metric='cosine': `bank` holds the L2-normalised rows.  image_scores: 'max' and 'reweighted'."""

    def store(self, det, bank) -> None:
        det.bank = ops.l2_normalize_rows(det._dev(bank))

    def scores(self, det, x):
        if x.shape[1] % 32 == 0 and 1 <= det.k <= 3:
            # normalise + similarity GEMM + k smallest distances in one kernel: no N x bank matrix in HBM (csrc/knn.hip)
            return ops.cosine_knn_fused(x, det.bank, det.k)
        qn = ops.l2_normalize_rows(x)
        out = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        step = 1 << 18
        for i in range(0, x.shape[0], step):
            sim = ops.linear_fwd(qn[i:i + step], det.bank)
            out[i:i + step] = ops.cosine_knn_mean(sim, det.k)
        return out

    def kneighbors(self, det, x, k):
        return ops.cosine_knn_index(x, det.bank, k)

    def reweight(self, det, xs, smax, neighbours):
        _, mstar = ops.cosine_knn_index(xs, det.bank, 1)                # m*: an index pass over one row per image
        centre = det.bank.index_select(0, mstar.reshape(-1).long())     # B_{m*}
        sim = ops.linear_fwd(centre, det.bank)                          # [batch][R] similarities of B_{m*} to the bank
        _, nbr = ops.rows_smallest_index(sim, neighbours, cosine=True)  # N: the rows nearest to B_{m*}
        return ops.knn_reweight(xs, det.bank, mstar, nbr, smax)


class FlatL2(SearchPath):
    """metric='euclidean', every query against every row: `bank` holds the raw fp32 rows, `bank_sq` their squared norms (recomputed by
    ``load``).  k <= 3 and 4..32 are two families of kernels.  image_scores: 'max' and 'reweighted'.  Also the base of the other
    Euclidean paths: the width check, and ``_set``, the one place that says what the bank is made of."""
    fused, index, topk_mean, topk_index = "l2_knn_fused", "l2_knn_index", "l2_topk_mean", "l2_topk_index"

    def _check_width(self, what, d) -> None:
        if d % 32:
            raise ValueError(f"{what}: metric='euclidean' needs an embedding width that is a multiple of 32, got {d}")

    def _set(self, det, rows) -> None:
        det.bank, det.bank_sq = rows, ops.row_sqnorms(rows)

    def store(self, det, bank) -> None:
        self._check_width("fit_bank", int(torch.as_tensor(bank).shape[1]))
        self._set(det, det._dev(bank))

    def keep(self, det, sel, rows) -> None:
        super().keep(det, sel, rows)
        det.bank_sq = det.bank_sq.index_select(0, sel).contiguous()

    def load(self, det, state) -> None:
        self._set(det, det._dev(state["bank"]))

    def scores(self, det, x):
        self._check_width("predict", x.shape[1])
        return getattr(ops, self.topk_mean if det.k > 3 else self.fused)(x, det.bank, det.bank_sq, det.k)

    def kneighbors(self, det, x, k):
        return getattr(ops, self.topk_index if k > 3 else self.index)(x, det.bank, det.bank_sq, k)

    def reweight(self, det, xs, smax, neighbours):
        _, mstar = ops.l2_knn_index(xs, det.bank, det.bank_sq, 1)
        rows = mstar.reshape(-1).long()
        dots = ops.linear_fwd(det.bank.index_select(0, rows), det.bank)                    # <B_{m*}, B_r>
        d2 = ops.l2_from_dots(dots, det.bank_sq.index_select(0, rows), det.bank_sq)
        _, nbr = ops.rows_smallest_index(d2, neighbours, cosine=False)
        return ops.knn_reweight_l2(xs, det.bank, mstar, nbr, smax)


class FlatL2Half(FlatL2):
    """bank_dtype='float16': `bank` holds the rows rounded to fp16, `bank_sq` the squared norms of the rounded rows.  ``load`` rounds the
    halves again: they are fixed points of the rounding, so it returns them and the norms in the fit's order.  image_scores: 'max'
    (check_bank_dtype refuses 'reweighted')."""
    fused, index, topk_mean, topk_index = "l2h_knn_fused", "l2h_knn_index", "l2h_topk_mean", "l2h_topk_index"

    def _set(self, det, rows) -> None:
        det.bank, det.bank_sq = ops.rows_to_half(rows)

    def state(self, det):
        return _state(det, bank_dtype='float16')


class FlatL2Int8(FlatL2):
    """bank_dtype='int8': `quant` = (lo, s) of the 8-bit code, lo / hi the smallest / largest element of the rows that are kept, `bank`
    the codes and `bank_sq` their int32 squared norms.  All three travel in a state as they are: nothing is recomputed, so nothing
    can differ between ranks.  k <= 3; image_scores: 'max'."""

    def _set(self, det, rows) -> None:
        lo, hi = torch.aminmax(rows)
        lo, s, inv_s, _ = ops.int8_quantiser(lo.item(), hi.item())
        det.bank, det.bank_sq, _ = ops.rows_to_int8(rows, lo, inv_s, s)
        det.quant = (lo, s)

    def keep(self, det, sel, rows) -> None:
        self._set(det, rows.index_select(0, sel).contiguous())         # the code spans the rows that are kept

    def state(self, det):
        return _state(det, bank_dtype='int8', bank_sq=det.bank_sq.cpu(), lo=det.quant[0], s=det.quant[1])

    def load(self, det, state) -> None:
        dev = det._dev(torch.zeros(1)).device
        det.bank = torch.as_tensor(state["bank"], dtype=torch.int8).to(dev).contiguous()
        det.bank_sq = torch.as_tensor(state["bank_sq"], dtype=torch.int32).to(dev).contiguous()
        det.quant = (float(state["lo"]), float(state["s"]))

    def scores(self, det, x):
        self._check_width("predict", x.shape[1])
        return ops.l2q_knn_fused(x, det.bank, det.bank_sq, det.quant, det.k)

    def kneighbors(self, det, x, k):
        return ops.l2q_knn_index(x, det.bank, det.bank_sq, det.quant, k)


class Refined:
    """refine=r on a compressed bank (faiss' IndexRefineFlat): the coarse bank of the class this is mixed into, and beside it
    `bank_f32`, the same rows as they were.  A query takes the coarse search's min(r, R) nearest rows as a shortlist (``_coarse``: the
    k <= 3 index kernel, or the list kernel from 4 on) and ranks them again by the direct fp32 distance to `bank_f32`
    (ops.l2_rerank_mean / l2_rerank_index): every distance returned is that to a real bank row.  `bank_f32` follows the bank through
    ``store``, ``keep``, ``state`` and ``load``."""

    def _set(self, det, rows) -> None:
        super()._set(det, rows)
        det.bank_f32 = rows

    def state(self, det):
        return dict(super().state(det), refine=det.refine, bank_f32=det.bank_f32.cpu())

    def load(self, det, state) -> None:
        super().load(det, state)
        det.bank_f32 = det._dev(state["bank_f32"])

    def _shortlist(self, det, what, x, k):
        rr = min(det.refine, int(det.bank.shape[0]))
        if k > rr:
            raise ValueError(f"{what}: refine={det.refine} on a bank of {int(det.bank.shape[0])} rows gives a shortlist of {rr} rows, "
                             f"fewer than k = {k}")
        return self._coarse(det, x, rr)[1]

    def scores(self, det, x):
        self._check_width("predict", x.shape[1])
        return ops.l2_rerank_mean(x, det.bank_f32, self._shortlist(det, "predict", x, det.k), det.k)

    def kneighbors(self, det, x, k):
        return ops.l2_rerank_index(x, det.bank_f32, self._shortlist(det, "kneighbors", x, k), k)


class RefinedHalf(Refined, FlatL2Half):
    """bank_dtype='float16', refine=r: the shortlist comes from l2h_knn_index / l2h_topk_index."""

    def keep(self, det, sel, rows) -> None:
        super().keep(det, sel, rows)
        det.bank_f32 = det.bank_f32.index_select(0, sel).contiguous()

    def load(self, det, state) -> None:
        FlatL2Half._set(self, det, det._dev(state["bank"]))            # the halves again, as FlatL2Half.load; not through Refined._set
        det.bank_f32 = det._dev(state["bank_f32"])

    def _coarse(self, det, x, r):
        return FlatL2Half.kneighbors(self, det, x, r)


class RefinedInt8(Refined, FlatL2Int8):
    """bank_dtype='int8', refine=r: the shortlist comes from l2q_knn_index / l2q_topk_index.  ``keep`` codes the kept rows again
    (FlatL2Int8.keep -> ``_set``), which keeps them as `bank_f32` too."""

    def _coarse(self, det, x, r):
        return (ops.l2q_topk_index if r > 3 else ops.l2q_knn_index)(x, det.bank, det.bank_sq, det.quant, r)


class Gallery(FlatL2):
    """gallery=K: the fp32 bank is made of whole images of `det.patches` rows; `bank_desc` holds their descriptors (recomputed by
    ``load``, and by ``retrieve`` after a bare ``fit_bank``).  k <= 3; image_scores: 'max' and 'retrieval'."""

    def store(self, det, bank) -> None:
        det._whole_images("fit_bank", int(torch.as_tensor(bank).shape[0]))
        det.bank_desc = None
        super().store(det, bank)

    def finish(self, det) -> None:
        det.bank_desc = ops.group_means(det.bank, det.patches)

    def state(self, det):
        return _state(det, gallery=det.gallery)

    def load(self, det, state) -> None:
        det._whole_images("load_state", int(state["bank"].shape[0]))
        super().load(det, state)
        self.finish(det)

    def retrieve(self, det, x):
        det._whole_images("predict", int(x.shape[0]))
        if det.bank_desc is None:
            self.finish(det)
        d2 = ops.l2_direct(ops.group_means(x, det.patches), det.bank_desc)
        vals, order = torch.sort(d2, dim=1, stable=True)
        kq = min(det.gallery, int(d2.shape[1]))
        return order[:, :kq].to(torch.int32).contiguous(), vals[:, :kq].contiguous()

    def scores(self, det, x):
        self._check_width("predict", x.shape[1])
        gallery, _ = self.retrieve(det, x)
        return ops.l2_knn_gallery(x, det.bank, det.bank_sq, gallery, det.patches, det.k)

    def kneighbors(self, det, x, k):
        gallery, _ = self.retrieve(det, x)
        return ops.l2_knn_gallery_index(x, det.bank, det.bank_sq, gallery, det.patches, k)


class IVF(FlatL2):
    """index='ivf': ``finish`` clusters the fp32 bank and keeps it sorted by cell; `ivf` holds perm, offsets, centroids, cent_sq, nlist
    and nprobe.  A state carries all but cent_sq, which ``load`` recomputes like `bank_sq`.  ``fit_bank`` alone builds no index.
    k <= 3; image_scores: 'max'."""

    def _index(self, det, what):
        if det.ivf is None:
            raise ValueError(f"{what}: index='ivf' has no index yet (fit first; fit_bank alone builds none)")
        return det.ivf

    def _set_index(self, det, perm, offsets, centroids, nlist, nprobe) -> None:
        det.ivf = {"perm": perm.contiguous(), "offsets": offsets.contiguous(), "centroids": centroids.contiguous(),
                   "cent_sq": ops.row_sqnorms(centroids), "nlist": int(nlist), "nprobe": int(nprobe)}

    def finish(self, det) -> None:
        """Clusters the bank rows and re-stores them cell after cell (stable in the caller's row order within a cell)."""
        from .models import ivf_nlist
        nlist = ivf_nlist(det.nlist, int(det.bank.shape[0]))
        centroids, assign = ops.kmeans_l2(det.bank, nlist, **det.index_options)
        sorted_cells, perm = torch.sort(assign, stable=True)
        self._set(det, det.bank.index_select(0, perm).contiguous())
        self._set_index(det, perm.to(torch.int32), ops.cell_offsets(sorted_cells, nlist), centroids, nlist, min(det.nprobe, nlist))

    def state(self, det):
        state = _state(det)
        ivf = self._index(det, "state")
        state.update({k: ivf[k].cpu() for k in ("perm", "offsets", "centroids")}, nlist=ivf["nlist"], nprobe=ivf["nprobe"])
        return state

    def load(self, det, state) -> None:
        super().load(det, state)
        dev = det.bank.device
        self._set_index(det, state["perm"].to(dev), state["offsets"].to(dev), state["centroids"].to(dev), state["nlist"], state["nprobe"])

    def _probed(self, det, what, x):
        """(offsets, probes, perm) of the queries x: the arguments of the index kernels after the bank."""
        ivf = self._index(det, what)
        return ivf["offsets"], ops.ivf_probes(x, ivf["centroids"], ivf["cent_sq"], ivf["nprobe"]), ivf["perm"]

    def scores(self, det, x):
        self._check_width("predict", x.shape[1])
        return ops.l2_knn_ivf(x, det.bank, det.bank_sq, *self._probed(det, "predict", x), det.k)

    def kneighbors(self, det, x, k):
        return ops.l2_knn_ivf_index(x, det.bank, det.bank_sq, *self._probed(det, "kneighbors", x), k)


_COSINE, _GALLERY, _IVF = Cosine(), Gallery(), IVF()
_FLAT = {'float32': FlatL2(), 'float16': FlatL2Half(), 'int8': FlatL2Int8()}
_REFINED = {'float16': RefinedHalf(), 'int8': RefinedInt8()}


def choose(metric, index, gallery, bank_dtype, refine=None) -> SearchPath:
    """The path of a detector with these (validated) options."""
    if metric == 'cosine':
        return _COSINE
    if gallery is not None:
        return _GALLERY
    if refine is not None:
        return _REFINED[bank_dtype]
    return _IVF if index == 'ivf' else _FLAT[bank_dtype]
