"""The reference of the LeCam regulariser (include/aclgan_hip.h: aclgan_ctx_set_lecam) for the tests: a replacement for the oracle's
module-level lsgan (monkeypatch.setattr(O, "lsgan", ...)) for ONE dis_losses call, and the fold of the anchors restated in Python floats.

oracle.dis_losses calls lsgan eight times in a fixed order; CALLS names the discriminator, the class (= the target: 0 the fake side, 1 the
real side) and the weight the caller multiplies the call's value with.  The wrapper leaves the VALUE of every call as it is -- the 16
losses keep their meaning -- and adds lam * sum_s mean((o_s - a[D][s][1 - class])^2) to its GRADIENT (the anchors are constants); it records
the per-scale means of the outputs and the per-scale values of the term."""
import torch

CALLS = [("A", 0, 0.5), ("A", 1, 0.5), ("A", 0, 0.5), ("A", 1, 0.5), ("B", 0, 1.0), ("B", 1, 1.0), ("2", 0, 1.0), ("2", 1, 1.0)]
NETS = ("A", "B", "2")


def oracle_lsgan(orig, anchors, lam):
    """anchors: {'A', 'B', '2'} -> num_scales rows of (fake anchor, real anchor), or None for an update with count == 0 (no term, the
    regulariser's values are 0).  lam: lam_eff of the update (0 before the start: the values are still recorded)."""
    rec = {"means": [], "terms": []}

    def wrapper(outs, target):
        k = len(rec["means"])
        assert k < len(CALLS), "dis_losses calls lsgan eight times"
        D, cls, _ = CALLS[k]
        assert float(target) == float(cls), (k, target)
        base = orig(outs, target)
        rec["means"].append([float(o.detach().double().mean()) for o in outs])
        if anchors is None:
            rec["terms"].append([0.0 for _ in outs])
            return base
        terms = [torch.mean((o - float(anchors[D][s][1 - cls])) ** 2) for s, o in enumerate(outs)]
        rec["terms"].append([float(t.detach()) for t in terms])
        reg = sum(terms)
        return base + lam * (reg - reg.detach())      # the value of the call stays; its gradient gains lam * d reg
    wrapper.rec = rec
    return wrapper


def lecam_values(rec):
    """{'A', 'B', '2'}: sum over the discriminator's calls of weight * sum over the scales of mean((o - a)^2) (without lambda)"""
    assert len(rec["terms"]) == len(CALLS)
    out = {D: 0.0 for D in NETS}
    for (D, _, w), terms in zip(CALLS, rec["terms"]):
        out[D] += w * sum(terms)
    return out


def class_means(rec):
    """{'A', 'B', '2'}: per scale [m_fake, m_real], each the weighted mean of the calls of that class"""
    assert len(rec["means"]) == len(CALLS)
    S = len(rec["means"][0])
    out = {}
    for D in NETS:
        rows = []
        for s in range(S):
            row = []
            for cls in (0, 1):
                sel = [(w, m[s]) for (d, c, w), m in zip(CALLS, rec["means"]) if d == D and c == cls]
                row.append(sum(w * v for w, v in sel) / sum(w for w, _ in sel))
            rows.append(row)
        out[D] = rows
    return out


def fold(anchors, means, count, decay):
    """the anchors after one more update: a copy of the means at count 0, else decay * a + (1 - decay) * m"""
    if count == 0:
        return {D: [list(r) for r in means[D]] for D in NETS}
    return {D: [[decay * a + (1.0 - decay) * m for a, m in zip(ra, rm)] for ra, rm in zip(anchors[D], means[D])] for D in NETS}
