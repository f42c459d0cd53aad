"""gen_update adopts the content encodings of x_a that the dis_update before it computed (aclgan_ctx_carry_encodings).

Both updates open with encode(gen_AB, x_a) and encode(gen_BA, x_a), and dis_update leaves the generators alone, so the adopted tensors are
the ones gen_update would compute: with the reuse on and off,
  * the deterministic plan gives the same bits -- all 16 losses, every gradient and every parameter after Adam of both groups, over two
    chained steps (the second shows that the carry region is rewritten and survives reuse), fp32 and bf16, with 1 and 3 lanes;
  * the default plan (fp32 atomics in a few reductions) agrees within the un-frozen gradient bound of tests/test_gpu_fullsize.py (GTOL);
  * whenever anything the encodings depend on may have changed -- x_a written or replaced, the generators stepped or reloaded, another
    batch size, no dis_update before, a captured update, masks being recorded -- nothing is adopted and the results are those of the
    reuse-off run on the same inputs.
Fixture: the reduced-width networks (dim 16, 2 ResBlocks) at 64x64 B=2, and one non-square 64x96 B=1 (ragged carry sizes)."""
import ctypes as C

import pytest
import torch

from oracle import aclgan_oracle as O
from test_gpu_fullsize import GTOL, LTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import aclgan_amd  # noqa: F401
    from aclgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def fix():
    cfg = O.default_config()
    cfg["gen"].update(dim=16, mlp_dim=32, n_res=2); cfg["dis"].update(dim=16)
    cfg["display_size"] = 1
    cfg["focus_epsilon"] = 0.5
    return cfg, O.test_nets(cfg, 0)


@pytest.fixture()
def tuning(L):
    """set tuning keys for one test; restored afterwards, with the process-wide deterministic mode"""
    saved = {}
    det = L.lib.aclgan_get_deterministic()

    def set_(key, value):
        prev = C.c_int()
        L.check(L.lib.aclgan_tuning(key.encode(), value, C.byref(prev)), "tuning")
        saved.setdefault(key, prev.value)
    yield set_
    for key, value in saved.items():
        L.check(L.lib.aclgan_tuning(key.encode(), value, None), "tuning")
    L.check(L.lib.aclgan_set_deterministic(det))


def _hits(L):
    v = C.c_longlong()
    L.check(L.lib.aclgan_tuning_get(b"enc_reuse_hits", C.byref(v)))
    return v.value


def _trainer(fix, **kw):
    from aclgan_amd.trainer import aclgan_Trainer
    cfg, nets = fix
    tr = aclgan_Trainer(cfg, **kw)
    for name in O.OracleTrainer.NETS:
        getattr(tr, name).load_state_dict(nets[name], strict=False)
    return tr


def _inputs(B, H, W, seed=5, steps=2):
    g = torch.Generator().manual_seed(seed)
    x_a = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    x_b = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    zs = [[torch.randn(B, 8, 1, 1, generator=g) for _ in range(6)] for _ in range(steps)]
    return x_a, x_b, zs


def _snap(tr):
    """everything an update leaves behind: the 16 losses, both groups' gradients, both groups' parameters"""
    torch.cuda.synchronize()
    return [tr._losses.clone()] + [tr._grad[g].clone() for g in (0, 1)] + [tr._param[g].clone() for g in (0, 1)]


def _gen(L, tr, cfg, x_a, x_b, z):
    """one gen_update: (passes adopted, kernel launches)"""
    h0, l0 = _hits(L), L.lib.aclgan_launch_count()
    tr.gen_update(x_a, x_b, cfg, z=z)
    return _hits(L) - h0, L.lib.aclgan_launch_count() - l0


def _chain(L, fix, tuning, reuse, B=2, H=64, W=64, steps=2, **kw):
    """`steps` chained (dis_update, gen_update) iterations on one device batch: snapshots after every update, adoptions and launches per gen_update"""
    tuning("enc_reuse", reuse)
    cfg = fix[0]
    tr = _trainer(fix, **kw)
    x_a, x_b, zs = _inputs(B, H, W, steps=steps)
    snaps, hits, launches = [], [], []
    for it in range(steps):
        tr.dis_update(x_a, x_b, cfg, z=zs[it][:3])
        snaps.append(_snap(tr))
        h, n = _gen(L, tr, cfg, x_a, x_b, zs[it][3:])
        snaps.append(_snap(tr)); hits.append(h); launches.append(n)
    return snaps, hits, launches


def _assert_same_bits(a, b):
    names = ("losses", "grad gen", "grad dis", "param gen", "param dis")
    for i, (sa, sb) in enumerate(zip(a, b)):
        for n, ta, tb in zip(names, sa, sb):
            assert torch.equal(ta, tb), ("update %d" % i, n, (ta - tb).abs().max().item())


def _assert_adopts_bit_for_bit(L, fix, tuning, **kw):
    on, hits_on, launches_on = _chain(L, fix, tuning, 1, deterministic=True, **kw)
    off, hits_off, launches_off = _chain(L, fix, tuning, 0, deterministic=True, **kw)
    print("adopted passes per gen_update on / off:", hits_on, hits_off, " launches per gen_update on / off:", launches_on, launches_off)
    assert hits_on == [2, 2] and hits_off == [0, 0]
    assert all(a < b for a, b in zip(launches_on, launches_off)), (launches_on, launches_off)
    _assert_same_bits(on, off)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 64, 96)])
def test_deterministic_plan_same_bits_with_and_without_reuse(L, fix, tuning, dtype, shape):
    B, H, W = shape
    _assert_adopts_bit_for_bit(L, fix, tuning, B=B, H=H, W=W, compute_dtype=dtype)


@pytest.mark.parametrize("lanes", [1, 3])
def test_adopted_tensors_carry_lane_stamps(L, fix, tuning, lanes):
    """one lane and three: consumers of an adopted tensor on another lane wait as they would for a computed one"""
    tuning("lanes", lanes)
    _assert_adopts_bit_for_bit(L, fix, tuning)


def test_default_plan_agrees_within_the_unfrozen_gradient_bound(L, fix, tuning):
    on, hits_on, _ = _chain(L, fix, tuning, 1, steps=1, deterministic=False)
    off, hits_off, _ = _chain(L, fix, tuning, 0, steps=1, deterministic=False)
    assert hits_on == [2] and hits_off == [0]
    cfg = fix[0]
    from aclgan_amd.trainer import aclgan_Trainer      # (tensor layout of the flat gradient buffers)
    tr = aclgan_Trainer(cfg)
    for upd, grp in ((0, 1), (1, 0)):
        ga, gb = on[upd][1 + grp].double(), off[upd][1 + grp].double()
        worst = 0.0
        gmax = max(float(gb[e["offset"]: e["offset"] + e["numel"]].norm()) for e in tr._tensors[grp])
        for e in tr._tensors[grp]:
            a, b = ga[e["offset"]: e["offset"] + e["numel"]], gb[e["offset"]: e["offset"] + e["numel"]]
            if float(b.norm()) >= 1e-3 * gmax:      # (the floor of tests/test_gpu_fullsize.py: FLOOR)
                worst = max(worst, float((a - b).norm() / b.norm()))
        print("default plan, reuse on vs off, group %d: worst per-tensor relative L2 of the gradients %.3e" % (grp, worst))
        assert worst <= GTOL, (grp, worst)
        la, lb = on[upd][0].double(), off[upd][0].double()
        assert float(((la - lb).abs() / lb.abs().clamp_min(1e-3)).max()) <= LTOL


def _expect_no_adoption(L, fix, tuning, between, first=("dis",), trainer_kw=None, before=None):
    """`first` updates, then between(tr, x_a, x_b) -> the (x_a, x_b) of the gen_update under test: it adopts nothing, and leaves what a
    trainer with the reuse off leaves after the same calls"""
    cfg = fix[0]
    out = []
    for reuse in (1, 0):
        tuning("enc_reuse", reuse)
        tr = _trainer(fix, deterministic=True, **(trainer_kw or {}))
        x_a, x_b, zs = _inputs(2, 64, 64, steps=3)
        if before is not None:
            before(tr)
        for i, which in enumerate(first):
            if which == "dis":
                tr.dis_update(x_a, x_b, cfg, z=zs[i][:3])
            else:
                tr.gen_update(x_a, x_b, cfg, z=zs[i][3:])
        xa2, xb2 = between(tr, x_a, x_b)
        h, _ = _gen(L, tr, cfg, xa2, xb2, [t[:xa2.shape[0]] for t in zs[2][3:]])
        assert h == 0, (reuse, h)
        out.append(_snap(tr))
    _assert_same_bits([out[0]], [out[1]])


def test_version_bump_of_x_a_is_not_adopted(L, fix, tuning):
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a.add_(0), b))


def test_modified_x_a_is_not_adopted(L, fix, tuning):
    """the case a stale adoption would fail: the result is the reuse-off run's on the MODIFIED image"""
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a.mul_(0.5), b))


def test_another_tensor_with_the_same_contents_is_not_adopted(L, fix, tuning):
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a.clone(), b))


def test_second_gen_update_in_a_row_is_not_adopted(L, fix, tuning):
    """D1:G2 cadence: the second gen_update follows the generators' Adam step"""
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a, b), first=("dis", "gen"))


def test_load_state_dict_between_the_updates_is_not_adopted(L, fix, tuning):
    def reload(tr, a, b):
        tr.gen_AB.load_state_dict(O.test_nets(fix[0], 3)["gen_AB"], strict=False)
        return a, b
    _expect_no_adoption(L, fix, tuning, reload)


def test_changed_batch_size_is_not_adopted(L, fix, tuning):
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a[:1], b[:1]))


def test_gen_update_without_dis_update_is_not_adopted(L, fix, tuning):
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a, b), first=())


def test_hip_graph_trainer_is_not_adopted(L, fix, tuning):
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a, b), trainer_kw={"hip_graph": True})


def test_mask_capture_is_not_adopted(L, fix, tuning):
    keep = []

    def capture(tr):
        buf = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
        keep.append(buf)
        L.check(L.lib.aclgan_debug_capture_masks(tr._ctx, L.ptr(buf), buf.numel()), "debug_capture_masks")
    _expect_no_adoption(L, fix, tuning, lambda tr, a, b: (a, b), before=capture)


def test_second_dis_update_is_the_one_adopted(L, fix, tuning):
    """dis_update, dis_update, gen_update: the record is the SECOND dis_update's (the first one's is dropped, the region rewritten)"""
    cfg = fix[0]
    out = []
    for reuse in (1, 0):
        tuning("enc_reuse", reuse)
        tr = _trainer(fix, deterministic=True)
        x_a, x_b, zs = _inputs(2, 64, 64, steps=2)
        x_a2 = x_a.flip(0).contiguous()
        tr.dis_update(x_a, x_b, cfg, z=zs[0][:3])
        tr.dis_update(x_a2, x_b, cfg, z=zs[1][:3])
        h, _ = _gen(L, tr, cfg, x_a2, x_b, zs[1][3:])
        assert h == (2 if reuse else 0)
        out.append(_snap(tr))
    _assert_same_bits([out[0]], [out[1]])
