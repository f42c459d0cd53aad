"""Every *_from_config of the trainer module on a literal list of configs, against tests/golden/config_keys.json: per config and function the
repr of the result or the exact exception message.  The fixture pins what a move of the validators must keep: every message byte for byte,
and which key is reported first when two are wrong.  It is recorded by this module's own recorder (python tests/test_config_keys_cpu.py
--record) and is only recorded again when a message or a default changes on purpose."""
import copy
import ctypes as C
import json
import os
import sys

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "config_keys.json")
FUNCS = ("dis_norm_from_config", "arch_from_config", "ema_from_config", "augment_from_config", "r1_from_config", "lecam_from_config",
         "ada_from_config", "modeseek_from_config", "grad_clip_from_config", "hparams_from_config")
INF, NAN = float("inf"), float("nan")

BASE = {"input_dim_a": 3, "input_dim_b": 3, "display_size": 1,
        "gen": {"dim": 8, "mlp_dim": 16, "style_dim": 8, "output_dim": 4, "n_downsample": 2, "n_res": 2, "activ": "relu", "pad_type": "reflect"},
        "dis": {"dim": 8, "n_layer": 4, "num_scales": 3, "activ": "lrelu", "pad_type": "reflect", "gan_type": "lsgan", "norm": "none"},
        "gan_w": 1, "gan_cw": 0.5, "recon_x_w": 10, "focus_loss": 0.025, "focus_delta": 7, "focus_upper": 3, "focus_lower": 0.5,
        "focus_epsilon": 0.01, "alpha": 1}
AUG = {"dis_augment": "color,translation,cutout"}
ADAPTIVE = {"dis_augment": "color", "dis_augment_p": "adaptive"}


def _a(**kw):
    return dict(ADAPTIVE, **kw)


# (name, keys laid over BASE; "gen" / "dis" / "drop" are special: sub-dict updates and top-level keys to remove)
CASES = [
    ("default", {}),
    ("empty_dict_no_base", None),      # {} itself: the validators that read top-level keys only take it, the others name the missing key
    # ---- dis.norm and the architecture ----
    ("dis_norm_absent", {"drop_dis": ["norm"]}),
    ("dis_norm_sn", {"dis": {"norm": "sn"}}),
    ("dis_norm_unknown", {"dis": {"norm": "bn"}}),
    ("dis_norm_none_object", {"dis": {"norm": None}}),
    ("gen_activ_wrong", {"gen": {"activ": "lrelu"}}),
    ("gen_pad_wrong", {"gen": {"pad_type": "zero"}}),
    ("gen_activ_pad_absent", {"drop_gen": ["activ", "pad_type"]}),
    ("dis_activ_wrong", {"dis": {"activ": "relu"}}),
    ("dis_pad_wrong", {"dis": {"pad_type": "zero"}}),
    ("dis_gan_type_wrong", {"dis": {"gan_type": "nsgan"}}),
    ("arch_two_wrong_gen_first", {"gen": {"pad_type": "zero"}, "dis": {"activ": "relu"}}),
    ("arch_two_wrong_activ_before_norm", {"dis": {"gan_type": "hinge", "norm": "bn"}}),
    ("arch_float_and_string_dims", {"gen": {"dim": 8.0, "n_res": "2"}, "input_dim_a": "3"}),
    ("arch_missing_dim", {"drop_gen": ["dim"]}),
    # ---- ema ----
    ("ema_decay_0", {"ema_decay": 0}),
    ("ema_decay_high", {"ema_decay": 0.9999}),
    ("ema_decay_int_true_zero_float", {"ema_decay": 0.0, "ema_start": 0, "ema_display": False}),
    ("ema_decay_rounds_to_1_in_fp32", {"ema_decay": 0.99999999}),
    ("ema_decay_1", {"ema_decay": 1}),
    ("ema_decay_negative", {"ema_decay": -0.1}),
    ("ema_decay_bool", {"ema_decay": True}),
    ("ema_decay_string", {"ema_decay": "0.9"}),
    ("ema_decay_none", {"ema_decay": None}),
    ("ema_decay_nan", {"ema_decay": NAN}),
    ("ema_decay_inf", {"ema_decay": INF}),
    ("ema_decay_overflow", {"ema_decay": 1e39}),
    ("ema_start_valid", {"ema_decay": 0.9, "ema_start": 1000}),
    ("ema_start_large", {"ema_decay": 0.9, "ema_start": 2 ** 40}),
    ("ema_start_negative", {"ema_start": -1}),
    ("ema_start_bool", {"ema_start": True}),
    ("ema_start_float", {"ema_start": 2.0}),
    ("ema_start_string", {"ema_start": "3"}),
    ("ema_display_on", {"ema_decay": 0.9, "ema_display": True}),
    ("ema_display_without_decay", {"ema_display": True}),
    ("ema_display_int", {"ema_decay": 0.9, "ema_display": 1}),
    ("ema_display_string", {"ema_decay": 0.9, "ema_display": "true"}),
    ("ema_two_wrong_decay_first", {"ema_decay": 2, "ema_start": -1}),
    ("ema_two_wrong_start_before_display", {"ema_start": 1.5, "ema_display": "yes"}),
    # ---- dis_augment ----
    ("aug_empty", {"dis_augment": ""}),
    ("aug_blank", {"dis_augment": "   "}),
    ("aug_color", {"dis_augment": "color"}),
    ("aug_translation", {"dis_augment": "translation"}),
    ("aug_cutout", {"dis_augment": "cutout"}),
    ("aug_all", AUG),
    ("aug_spaces_and_order", {"dis_augment": " cutout , color "}),
    ("aug_twice", {"dis_augment": "color,cutout,color"}),
    ("aug_unknown", {"dis_augment": "color,blur"}),
    ("aug_empty_name", {"dis_augment": "color,,cutout"}),
    ("aug_upper_case", {"dis_augment": "Color"}),
    ("aug_unknown_before_twice", {"dis_augment": "blur,color,color"}),
    ("aug_int", {"dis_augment": 7}),
    ("aug_bool", {"dis_augment": True}),
    ("aug_none", {"dis_augment": None}),
    ("aug_list", {"dis_augment": ["color"]}),
    # ---- r1 ----
    ("r1_gamma_0", {"r1_gamma": 0}),
    ("r1_gamma_10", {"r1_gamma": 10}),
    ("r1_gamma_tiny", {"r1_gamma": 1e-30, "r1_every": 1}),
    ("r1_gamma_fp32_max", {"r1_gamma": 3.4e38, "r1_every": 1}),
    ("r1_gamma_overflow", {"r1_gamma": 1e39}),
    ("r1_gamma_negative", {"r1_gamma": -1}),
    ("r1_gamma_bool", {"r1_gamma": True}),
    ("r1_gamma_string", {"r1_gamma": "10"}),
    ("r1_gamma_none", {"r1_gamma": None}),
    ("r1_gamma_nan", {"r1_gamma": NAN}),
    ("r1_gamma_inf", {"r1_gamma": INF}),
    ("r1_every_1", {"r1_gamma": 10, "r1_every": 1}),
    ("r1_every_large", {"r1_gamma": 1e-3, "r1_every": 2 ** 31}),
    ("r1_every_0", {"r1_every": 0}),
    ("r1_every_negative", {"r1_gamma": 10, "r1_every": -4}),
    ("r1_every_bool", {"r1_every": True}),
    ("r1_every_float", {"r1_every": 16.0}),
    ("r1_every_string", {"r1_every": "16"}),
    ("r1_product_overflow", {"r1_gamma": 3e38, "r1_every": 16}),
    ("r1_product_overflow_off", {"r1_gamma": 0, "r1_every": 2 ** 200}),
    ("r1_with_sn", {"r1_gamma": 10, "dis": {"norm": "sn"}}),
    ("r1_off_with_sn", {"r1_gamma": 0, "dis": {"norm": "sn"}}),
    ("r1_with_augment", dict(AUG, r1_gamma=10)),
    ("r1_off_with_augment", dict(AUG, r1_gamma=0)),
    ("r1_with_sn_and_augment_sn_first", dict(AUG, r1_gamma=10, dis={"norm": "sn"})),
    ("r1_with_bad_augment", {"r1_gamma": 10, "dis_augment": "blur"}),
    ("r1_off_with_bad_augment", {"r1_gamma": 0, "dis_augment": "blur"}),
    ("r1_two_wrong_gamma_first", {"r1_gamma": -1, "r1_every": 0}),
    ("r1_two_wrong_every_before_sn", {"r1_gamma": 10, "r1_every": 0, "dis": {"norm": "sn"}}),
    ("r1_two_wrong_product_before_sn", {"r1_gamma": 3e38, "r1_every": 16, "dis": {"norm": "sn"}}),
    # ---- lecam ----
    ("lecam_lambda_0", {"lecam_lambda": 0}),
    ("lecam_lambda_1", {"lecam_lambda": 1}),
    ("lecam_lambda_fp32_max", {"lecam_lambda": 3.4e38}),
    ("lecam_lambda_overflow", {"lecam_lambda": 1e39}),
    ("lecam_lambda_negative", {"lecam_lambda": -0.0001}),
    ("lecam_lambda_bool", {"lecam_lambda": True}),
    ("lecam_lambda_string", {"lecam_lambda": "0.3"}),
    ("lecam_lambda_none", {"lecam_lambda": None}),
    ("lecam_lambda_nan", {"lecam_lambda": NAN}),
    ("lecam_lambda_inf", {"lecam_lambda": INF}),
    ("lecam_decay_0", {"lecam_lambda": 1, "lecam_decay": 0}),
    ("lecam_decay_high", {"lecam_lambda": 1, "lecam_decay": 0.9999}),
    ("lecam_decay_rounds_to_1_in_fp32", {"lecam_decay": 0.99999999}),
    ("lecam_decay_1", {"lecam_decay": 1}),
    ("lecam_decay_negative", {"lecam_decay": -0.1}),
    ("lecam_decay_bool", {"lecam_decay": False}),
    ("lecam_decay_string", {"lecam_decay": "0.99"}),
    ("lecam_decay_nan", {"lecam_decay": NAN}),
    ("lecam_start_0", {"lecam_lambda": 1, "lecam_start": 0}),
    ("lecam_start_max", {"lecam_lambda": 1, "lecam_start": 2 ** 31 - 1}),
    ("lecam_start_too_large", {"lecam_start": 2 ** 31}),
    ("lecam_start_negative", {"lecam_start": -1}),
    ("lecam_start_bool", {"lecam_start": True}),
    ("lecam_start_float", {"lecam_start": 1000.0}),
    ("lecam_start_string", {"lecam_start": "1000"}),
    ("lecam_two_wrong_lambda_first", {"lecam_lambda": -1, "lecam_decay": 1}),
    ("lecam_two_wrong_decay_before_start", {"lecam_decay": 1.5, "lecam_start": -1}),
    ("lecam_with_everything", dict(AUG, lecam_lambda=2.0, ema_decay=0.999, dis={"norm": "sn"})),
    # ---- dis_augment_p and the controller ----
    ("ada_p_0", dict(AUG, dis_augment_p=0)),
    ("ada_p_1", dict(AUG, dis_augment_p=1)),
    ("ada_p_half", dict(AUG, dis_augment_p=0.5)),
    ("ada_p_adaptive", ADAPTIVE),
    ("ada_p_adaptive_spaces", {"dis_augment": "color", "dis_augment_p": " adaptive "}),
    ("ada_p_adaptive_upper_case", {"dis_augment": "color", "dis_augment_p": "Adaptive"}),
    ("ada_p_other_string", {"dis_augment": "color", "dis_augment_p": "0.5"}),
    ("ada_p_negative", dict(AUG, dis_augment_p=-0.1)),
    ("ada_p_above_1", dict(AUG, dis_augment_p=1.0001)),
    ("ada_p_bool", dict(AUG, dis_augment_p=True)),
    ("ada_p_none", dict(AUG, dis_augment_p=None)),
    ("ada_p_nan", dict(AUG, dis_augment_p=NAN)),
    ("ada_p_inf", dict(AUG, dis_augment_p=INF)),
    ("ada_p_without_augment", {"dis_augment_p": 0.5}),
    ("ada_adaptive_without_augment", {"dis_augment_p": "adaptive", "dis_augment": " "}),
    ("ada_p_with_bad_augment", {"dis_augment_p": 0.5, "dis_augment": "blur"}),
    ("ada_two_wrong_p_before_augment", {"dis_augment_p": 2}),
    ("ada_keys_without_p", dict(AUG, ada_target=7, ada_interval=0, ada_kimg=-1)),
    ("ada_keys_ignored_with_fixed_p", dict(AUG, dis_augment_p=0.25, ada_target=7, ada_interval=0, ada_kimg=-1)),
    ("ada_target_low", _a(ada_target=-1)),
    ("ada_target_high", _a(ada_target=1)),
    ("ada_target_above", _a(ada_target=1.5)),
    ("ada_target_below", _a(ada_target=-1.5)),
    ("ada_target_bool", _a(ada_target=True)),
    ("ada_target_string", _a(ada_target="0.6")),
    ("ada_target_nan", _a(ada_target=NAN)),
    ("ada_interval_1", _a(ada_interval=1)),
    ("ada_interval_max", _a(ada_interval=2 ** 31 - 1)),
    ("ada_interval_0", _a(ada_interval=0)),
    ("ada_interval_too_large", _a(ada_interval=2 ** 31)),
    ("ada_interval_bool", _a(ada_interval=True)),
    ("ada_interval_float", _a(ada_interval=4.0)),
    ("ada_interval_string", _a(ada_interval="4")),
    ("ada_kimg_small", _a(ada_kimg=1e-3)),
    ("ada_kimg_int", _a(ada_kimg=100)),
    ("ada_kimg_fp32_max", _a(ada_kimg=3.4e38)),
    ("ada_kimg_0", _a(ada_kimg=0)),
    ("ada_kimg_negative", _a(ada_kimg=-500)),
    ("ada_kimg_overflow", _a(ada_kimg=1e39)),
    ("ada_kimg_inf", _a(ada_kimg=INF)),
    ("ada_kimg_nan", _a(ada_kimg=NAN)),
    ("ada_kimg_bool", _a(ada_kimg=True)),
    ("ada_kimg_string", _a(ada_kimg="500")),
    ("ada_two_wrong_target_first", _a(ada_target=2, ada_interval=0)),
    ("ada_two_wrong_interval_before_kimg", _a(ada_interval=0, ada_kimg=0)),
    ("ada_all_valid", _a(ada_target=0.5, ada_interval=8, ada_kimg=100.0)),
    # ---- ms_lambda ----
    ("ms_lambda_0", {"ms_lambda": 0}),
    ("ms_lambda_1", {"ms_lambda": 1}),
    ("ms_lambda_fp32_max", {"ms_lambda": 3.4e38}),
    ("ms_lambda_overflow", {"ms_lambda": 1e39}),
    ("ms_lambda_negative", {"ms_lambda": -1}),
    ("ms_lambda_bool", {"ms_lambda": True}),
    ("ms_lambda_string", {"ms_lambda": "1"}),
    ("ms_lambda_none", {"ms_lambda": None}),
    ("ms_lambda_nan", {"ms_lambda": NAN}),
    ("ms_lambda_inf", {"ms_lambda": INF}),
    # ---- grad_clip ----
    ("clip_0", {"grad_clip": 0}),
    ("clip_1", {"grad_clip": 1}),
    ("clip_inf", {"grad_clip": INF}),
    ("clip_overflow_is_inf", {"grad_clip": 1e39}),
    ("clip_underflow", {"grad_clip": 1e-50}),
    ("clip_smallest", {"grad_clip": 1e-45}),
    ("clip_negative", {"grad_clip": -1}),
    ("clip_bool", {"grad_clip": True}),
    ("clip_string", {"grad_clip": "1"}),
    ("clip_none", {"grad_clip": None}),
    ("clip_nan", {"grad_clip": NAN}),
    ("clip_gen_only", {"grad_clip_gen": 2.5}),
    ("clip_dis_only", {"grad_clip_dis": INF}),
    ("clip_gen_override_off", {"grad_clip": 1, "grad_clip_gen": 0}),
    ("clip_both_overrides", {"grad_clip": 1, "grad_clip_gen": 2, "grad_clip_dis": 3}),
    ("clip_gen_negative", {"grad_clip": 1, "grad_clip_gen": -2}),
    ("clip_dis_string", {"grad_clip_dis": "inf"}),
    ("clip_dis_underflow", {"grad_clip_dis": 1e-50}),
    ("clip_two_wrong_both_first", {"grad_clip": -1, "grad_clip_gen": True}),
    ("clip_two_wrong_gen_before_dis", {"grad_clip_gen": NAN, "grad_clip_dis": -1}),
    # ---- hparams ----
    ("hparams_alpha_absent", {"drop": ["alpha"]}),
    ("hparams_strings_that_parse", {"gan_w": "2", "focus_delta": "7.5"}),
    ("hparams_string_that_does_not", {"gan_cw": "half"}),
    ("hparams_missing_key", {"drop": ["recon_x_w"]}),
    ("hparams_two_missing_first_in_order", {"drop": ["focus_upper", "gan_cw"]}),
    ("hparams_focus_off", {"focus_loss": 0}),
    # ---- the stacks of tests/combo_ref.py and keys across validators ----
    ("stack_a", dict(AUG, dis_augment_p=0.5, lecam_lambda=1.0, lecam_start=0, lecam_decay=0.9, ms_lambda=32.0, grad_clip=1.0, ema_decay=0.9)),
    ("stack_b", dict(r1_gamma=40.0, r1_every=1, lecam_lambda=1.0, lecam_start=0, lecam_decay=0.9, ms_lambda=32.0, grad_clip=1.0, ema_decay=0.9)),
    ("one_wrong_key_per_validator", {"ema_decay": 1, "dis_augment": "blur", "r1_every": 0, "lecam_start": -1, "dis_augment_p": 2, "ms_lambda": -1,
                                     "grad_clip": -1, "dis": {"norm": "bn"}}),
]


def config_of(over):
    if over is None:
        return {}
    cfg = copy.deepcopy(BASE)
    for k, v in over.items():
        if k in ("gen", "dis"):
            cfg[k].update(v)
        elif k in ("drop_gen", "drop_dis"):
            for name in v:
                del cfg[k[5:]][name]
        elif k == "drop":
            for name in v:
                del cfg[name]
        else:
            cfg[k] = v
    return cfg


def show(v):
    """repr, with a ctypes structure (Arch, HParams) written as its fields"""
    if isinstance(v, C.Structure):
        return "%s(%s)" % (type(v).__name__, ", ".join("%s=%r" % (f[0], getattr(v, f[0])) for f in v._fields_))
    return repr(v)


def observe(T):
    out = {}
    for name, over in CASES:
        row = {}
        for fn in FUNCS:
            try:
                row[fn] = ["ok", show(getattr(T, fn)(config_of(over)))]
            except Exception as e:      # noqa: BLE001  (the type and the message are what the fixture holds)
                row[fn] = [type(e).__name__, str(e)]
        out[name] = row
    return out


def _trainer_module():
    import aclgan_amd  # noqa: F401
    from aclgan_amd import trainer
    return trainer


def test_case_names_are_unique_and_the_fixture_holds_exactly_them():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names)
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(names)
    assert all(sorted(row) == sorted(FUNCS) for row in want.values())


def test_every_result_and_every_message_is_the_recorded_one():
    T = _trainer_module()
    assert all(fn in T.__all__ for fn in FUNCS)
    with open(FIXTURE) as f:
        want = json.load(f)
    got = observe(T)
    wrong = [(name, fn, got[name][fn], want[name][fn]) for name, _ in CASES for fn in FUNCS if got[name][fn] != want[name][fn]]
    assert not wrong, wrong[:5]


def test_the_fixture_distinguishes_what_it_is_meant_to():
    """the recorded rows are not vacuous: every validator both accepts and refuses somewhere, and the two-wrong-keys rows name the first key"""
    with open(FIXTURE) as f:
        want = json.load(f)
    for fn in FUNCS:
        kinds = {row[fn][0] for row in want.values()}
        assert "ok" in kinds and len(kinds) > 1, fn
    first = {"ema_two_wrong_decay_first": ("ema_from_config", "ema_decay="), "ema_two_wrong_start_before_display": ("ema_from_config", "ema_start="),
             "r1_two_wrong_gamma_first": ("r1_from_config", "r1_gamma="), "r1_two_wrong_every_before_sn": ("r1_from_config", "r1_every="),
             "r1_two_wrong_product_before_sn": ("r1_from_config", "r1_gamma * r1_every"), "r1_with_sn_and_augment_sn_first": ("r1_from_config", "r1_gamma > 0 with dis.norm"),
             "lecam_two_wrong_lambda_first": ("lecam_from_config", "lecam_lambda="), "lecam_two_wrong_decay_before_start": ("lecam_from_config", "lecam_decay="),
             "ada_two_wrong_p_before_augment": ("ada_from_config", "dis_augment_p=2: expected"), "ada_two_wrong_target_first": ("ada_from_config", "ada_target="),
             "ada_two_wrong_interval_before_kimg": ("ada_from_config", "ada_interval="), "clip_two_wrong_both_first": ("grad_clip_from_config", "grad_clip=-1"),
             "clip_two_wrong_gen_before_dis": ("grad_clip_from_config", "grad_clip_gen="), "arch_two_wrong_gen_first": ("arch_from_config", "gen.pad_type="),
             "arch_two_wrong_activ_before_norm": ("arch_from_config", "dis.gan_type=")}
    for name, (fn, start) in first.items():
        kind, text = want[name][fn]
        assert kind == "AclganError" and text.startswith(start), (name, kind, text)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_config_keys_cpu.py --record   (writes tests/golden/config_keys.json from the code as it stands)")
    with open(FIXTURE, "w") as f:
        json.dump(observe(_trainer_module()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d configs x %d functions -> %s" % (len(CASES), len(FUNCS), FIXTURE))
