"""The neural imitator (cpmppi_dense_*, model_folder.load_dense_model, train_imitator), the parts that need no GPU: the folder
reader against the reference's own C export, the round trip through train_imitator.write_model_folder, the settings read from the
shipped config_training.yml and their refusals, the normalisation rule, the exports / ABI / header text, the code objects of the
unit, and the reference tests/dense_ref.py against a hand-written loop in the order of C_implementation/network.c."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dense_ref as D  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKOUT = os.path.join(ROOT, "tests", "golden", "reference_checkout")
EXPORT = os.path.join(ROOT, "tests", "golden", "keras_dense_c_export.npz")
FOLDER_INPUTS = ["angleD", "angle_cos", "angle_sin", "position", "positionD", "target_equilibrium", "target_position"]


# ---------------------------------------------------------------------------------------------- 1. the folder reader
@pytest.mark.parametrize("source", ["keras", "ckpt"])
def test_golden_folder_equals_the_c_export_bit_for_bit(source):
    from cartpolesimulation_amd import model_folder as MF
    assert list(MF.DENSE_INPUTS) == FOLDER_INPUTS == MF.read_net_info(D.GOLDEN_FOLDER)["inputs"]
    m = MF.load_dense_model(D.GOLDEN_FOLDER, source)
    gold = np.load(EXPORT)
    for l in range(3):
        w, b = m[f"w{l + 1}"], m[f"b{l + 1}"]
        assert w.dtype == np.float32 and w.flags.c_contiguous
        assert np.array_equal(w, gold[f"kernel{l}"].T) and np.array_equal(b, gold[f"bias{l}"])      # (the folder's order IS the kernel's)
    assert [m[k].shape for k in MF.DENSE_KEYS] == list(MF.DENSE_SHAPES)
    assert np.array_equal(m["in_scale"], np.array([0.05440483, 1, 1, 5.05050516, 0.88866770, 1, 5.05050516], f32))
    assert np.array_equal(m["in_shift"], np.zeros(7, f32))
    assert np.array_equal(m["out_scale"], np.ones(1, f32)) and np.array_equal(m["out_shift"], np.zeros(1, f32))


def _copy_folder(tmp_path, name="Dense-7IN-32H1-32H2-1OUT-0", edit=None, drop=()):
    import shutil
    dst = tmp_path / name
    shutil.copytree(D.GOLDEN_FOLDER, dst)
    for f in drop:
        os.remove(dst / f)
    if edit is not None:
        p = dst / "Dense-7IN-32H1-32H2-1OUT-0.txt"
        p.write_text(edit(p.read_text()))
    return str(dst)


def test_checkpoint_pair_alone_and_default_order(tmp_path):
    from cartpolesimulation_amd.model_folder import load_dense_model
    only_ckpt = _copy_folder(tmp_path, drop=["Dense-7IN-32H1-32H2-1OUT-0.keras"])
    a, b = load_dense_model(only_ckpt), load_dense_model(D.GOLDEN_FOLDER)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    with pytest.raises(FileNotFoundError, match="'keras'"):
        load_dense_model(only_ckpt, "keras")


def test_inputs_and_normalisation_are_permuted_to_kernel_order(tmp_path):
    """A folder that lists its inputs in config_training.yml's order: the reader permutes w1's columns and the vectors."""
    from cartpolesimulation_amd.model_folder import DENSE_INPUTS, load_dense_model
    order = ["position", "positionD", "angle_cos", "angle_sin", "angleD", "target_equilibrium", "target_position"]
    folder = _copy_folder(tmp_path, edit=lambda t: t.replace(", ".join(FOLDER_INPUTS), ", ".join(order)))
    a_file = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], f32)
    with open(os.path.join(folder, "normalization_vec_a.csv"), "w") as fh:
        fh.write(",".join(repr(float(x)) for x in a_file) + "\n")
    m, gold = load_dense_model(folder), np.load(EXPORT)
    pin = [order.index(f) for f in DENSE_INPUTS]
    assert np.array_equal(m["w1"], gold["kernel0"].T[:, pin]) and np.array_equal(m["in_scale"], a_file[pin])
    assert np.array_equal(m["w2"], gold["kernel1"].T)


def test_reader_refuses_by_name(tmp_path):
    from cartpolesimulation_amd import model_folder as MF
    for i, (text, edit) in enumerate((("TYPE 'GRU'", lambda t: t.replace("TYPE:\nDense", "TYPE:\nGRU")),
                       ("NET NAME 'Dense-64H1'", lambda t: t.replace("NET NAME:\nDense-32H1-32H2", "NET NAME:\nDense-64H1")),
                       ("features", lambda t: t.replace("angleD, angle_cos", "angle, angle_cos")),
                       ("features", lambda t: t.replace("OUTPUTS:\nQ_calculated_offline", "OUTPUTS:\nQ, Q2")))):
        with pytest.raises(NotImplementedError, match=text):
            MF.load_dense_model(_copy_folder(tmp_path / str(i), edit=edit))
    with pytest.raises(NotImplementedError):                    # (and the GRU reader still refuses the Dense folder)
        MF.load_gru_model(D.GOLDEN_FOLDER)
    with pytest.raises(NotImplementedError, match="Dense layer 0"):
        MF.keras_dense_weights_to_model([np.zeros((7, 16)), np.zeros(16), np.zeros((16, 32)), np.zeros(32), np.zeros((32, 1)), np.zeros(1)])


def test_write_model_folder_round_trips_every_array(tmp_path):
    from cartpolesimulation_amd.model_folder import load_dense_model, read_net_info
    from cartpolesimulation_amd.train_imitator import write_model_folder
    model = D.random_model(5, norm=True)
    model["in_scale"][2] = f32(1.0) / f32(3.0)
    folder = write_model_folder(tmp_path / "Dense-7IN-32H1-32H2-1OUT-7", model, info={"post wash out length": 50})
    back = load_dense_model(folder)
    assert set(back) == set(model)
    for k in model:
        assert back[k].dtype == np.float32 and np.array_equal(back[k], model[k]), k
    info = read_net_info(folder)
    assert info["net_name"] == "Dense-32H1-32H2" and info["type"] == "Dense" and info["post_wash_out_length"] == "50"
    plain = {k: model[k] for k in D.KEYS}
    back = load_dense_model(write_model_folder(tmp_path / "plain", plain))
    assert "in_scale" not in back and all(np.array_equal(back[k], plain[k]) for k in plain)
    with pytest.raises(ValueError, match="weight w2 must have shape"):
        write_model_folder(tmp_path / "bad", {**plain, "w2": np.zeros((32, 16), f32)})


# ---------------------------------------------------------------------------------------------- 2. settings and normalisation
def training_config():
    import yaml
    with open(os.path.join(CHECKOUT, "SI_Toolkit_ASF", "config_training.yml")) as fh:
        return yaml.safe_load(fh)


def test_training_settings_takes_the_shipped_file_as_it_stands():
    from cartpolesimulation_amd.train_imitator import NET_NAME, training_settings
    settings, normalize = training_settings(training_config())
    assert NET_NAME == "Dense-32H1-32H2" and normalize is True
    assert settings == dict(epochs=30, batch_size=64, seed=1873, lr=2.0e-3, reduce_lr_on_plateau=True, patience=2, decrease_factor=0.5,
                            minimal_lr=1.0e-7, min_delta=1.0e-6, post_wash_out=1, shift_labels=0)
    settings, _ = training_settings(training_config(), epochs=3, lr=None, post_wash_out=50)
    assert settings["epochs"] == 3 and settings["lr"] == 2.0e-3 and settings["post_wash_out"] == 50


def test_training_settings_refuses_each_changed_key_by_name():
    from cartpolesimulation_amd.train_imitator import training_settings

    def refused(text, change, **kw):
        cfg = training_config()
        change(cfg)
        with pytest.raises(ValueError, match=text):
            training_settings(cfg, **kw)

    t = "training_default"
    refused("net 'GRU-32H1-32H2'", lambda c: c["modeling"].update(NET_NAME="GRU-32H1-32H2"))
    refused("net 'Dense-64H1-64H2'", lambda c: None, net="Dense-64H1-64H2")
    refused("inputs .*the seven inputs", lambda c: c[t].update(state_inputs=c[t]["state_inputs"][:-1]))
    refused("inputs .*'Q'", lambda c: c[t].update(control_inputs=["Q"]))
    refused("outputs \\['angle'\\]", lambda c: c[t].update(outputs=["angle"]))
    refused("outputs", lambda c: c[t].update(outputs=["Q_calculated", "Q"]))
    refused("translation_invariant_variables", lambda c: c[t].update(translation_invariant_variables=["position"]))
    refused("WASH_OUT_LEN = 5", lambda c: c[t].update(WASH_OUT_LEN=5))
    refused("REGULARIZATION.ACTIVATED", lambda c: c["REGULARIZATION"].update(ACTIVATED=True))
    refused("QUANTIZATION.ACTIVATED", lambda c: c["QUANTIZATION"].update(ACTIVATED=True))
    refused("PRUNING.ACTIVATED", lambda c: c["PRUNING"].update(ACTIVATED=True))
    refused("ON_FLY_DATA_GENERATION", lambda c: c[t].update(ON_FLY_DATA_GENERATION=True))
    refused("USE_NNI", lambda c: c[t].update(USE_NNI=True))
    refused("CONFIG_SERIES_MODIFICATION", lambda c: c["CONFIG_SERIES_MODIFICATION"].update(MODE="train_for_random_vertical_angle_shift"))
    refused("FILTERS", lambda c: c.update(FILTERS={"butter": 1}))
    refused("post_wash_out >= 1", lambda c: None, post_wash_out=0)
    # setpoint_inputs may carry target_position, as the file's comment allows: the seven inputs are the same
    cfg = training_config()
    cfg[t].update(state_inputs=cfg[t]["state_inputs"][:-1], setpoint_inputs=["target_position"])
    assert training_settings(cfg)[0]["seed"] == 1873


def test_the_other_trainers_still_refuse_the_dense_net_in_their_words():
    from cartpolesimulation_amd import fit_ode, train_gru
    with pytest.raises(ValueError, match="net 'Dense-32H1-32H2'.*built for GRU-32H1-32H2"):
        train_gru.training_settings(training_config(), dynamics_model=True)
    with pytest.raises(ValueError, match="Dense-32H1-32H2"):
        fit_ode.fit_settings(training_config())


def test_normalisation_rule():
    from cartpolesimulation_amd.train_imitator import normalization_from_recordings
    s, tp, te, lab = D.recordings(3, R=3, T=40)
    te[:] = 1.0                                                     # a target column that never varies: identity
    lengths = np.array([40, 25, 0])
    s[1, 25:], lab[1, 25:], tp[2] = 1e6, 1e6, 1e6                    # (rows past a recording's length do not count)
    n = normalization_from_recordings(s, tp, te, lab, lengths)
    keep = np.arange(40)[None, :] < lengths[:, None]
    cols = [s[:, :, c][keep] for c in (1, 2, 3, 4, 5)] + [te[keep], tp[keep]]
    for i, c in enumerate(cols):
        if i == 5:
            assert n["in_scale"][5] == 1.0 and n["in_shift"][5] == 0.0
            continue
        lo, hi = float(c.min()), float(c.max())
        assert n["in_scale"][i] == f32(2.0 / (hi - lo)) and n["in_shift"][i] == f32(-(hi + lo) / (hi - lo))
        z = n["in_scale"][i] * c + n["in_shift"][i]
        assert abs(z.min() + 1) < 1e-6 and abs(z.max() - 1) < 1e-6
    lo, hi = float(lab[keep].min()), float(lab[keep].max())
    assert n["out_scale"][0] == f32((hi - lo) / 2) and n["out_shift"][0] == f32((hi + lo) / 2)
    assert all(n[k].dtype == np.float32 for k in n)
    tp[:] = 0.25                                                    # both targets constant: both identity
    n = normalization_from_recordings(s, tp, te, lab, lengths)
    assert n["in_scale"][6] == 1.0 and n["in_shift"][6] == 0.0
    with pytest.raises(ValueError, match="the label.*never vary"):
        normalization_from_recordings(s, tp, te, np.full_like(lab, 0.3), lengths)
    s2 = s.copy()
    s2[:, :, 4] = 0.1
    with pytest.raises(ValueError, match="'position'.*never vary"):
        normalization_from_recordings(s2, tp, te, lab, lengths)


def test_initial_weights_rule():
    from cartpolesimulation_amd.train_imitator import initial_weights
    a, b = initial_weights(1873), initial_weights(1873)
    assert all(np.array_equal(a[k], b[k]) for k in a) and list(a) == list(D.KEYS)
    rng = np.random.default_rng(1873)
    for k, shp in zip(D.KEYS, D.SHAPES):
        bound = 1.0 / np.sqrt(7.0 if k in ("w1", "b1") else 32.0)
        assert np.array_equal(a[k], rng.uniform(-bound, bound, size=shp).astype(f32))
        assert a[k].shape == shp and np.abs(a[k]).max() <= bound
    assert not np.array_equal(a["w2"], initial_weights(1874)["w2"])


# ---------------------------------------------------------------------------------------------- 3. exports, ABI, header, unit
NAMES = ("cpmppi_set_dense", "cpmppi_dense_control", "cpmppi_dense_train_reserve", "cpmppi_dense_loss_grad", "cpmppi_dense_train_begin",
         "cpmppi_dense_train_step", "cpmppi_dense_train_get")


def test_exports_abi_and_header_text():
    from cartpolesimulation_amd import _lib as L
    assert all(n in L.EXPORTS for n in NAMES)
    assert L.ABI_VERSION == 5 and L.DENSE_PARAMS == 1345 == D.NPAR == sum(int(np.prod(s)) for s in D.SHAPES)
    with open(os.path.join(ROOT, "include", "cpmppi.h")) as fh:
        header = fh.read()
    assert "#define CPMPPI_ABI_VERSION 5u" in header and "#define CPMPPI_DENSE_PARAMS 1345u" in header
    version_comment = header[header.index("#define CPMPPI_ABI_VERSION"):header.index("#define CPMPPI_STATE_DIM")]
    assert "cpmppi_set_dense / cpmppi_dense_model" in version_comment
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(cpmppi_handle\* h", header), n
        assert len(re.findall(r"\b" + n + r"\b", header)) >= 2, n      # declared, and spoken of in the text above
    assert "w1[32,7] b1[32] w2[32,32] b2[32] w3[1,32] b3[1]" in header
    assert "angleD, angle_cos, angle_sin, position, positionD,\n * target_equilibrium, target_position" in header
    assert "THIS LIBRARY'S OWN" in header[header.index("The NEURAL IMITATOR"):header.index("#define CPMPPI_DENSE_PARAMS")]
    if os.path.exists(L.LIB_PATH):
        assert L.load().cpmppi_abi_version() == 5
    for struct, name in ((L.cpmppi_dense_model, "cpmppi_dense_model"), (L.cpmppi_dense_control_args, "cpmppi_dense_control_args"),
                         (L.cpmppi_dense_loss_args, "cpmppi_dense_loss_args")):
        body = header[:header.index("} " + name + ";")]
        body = body[body.rindex("typedef struct {"):]
        fields = re.findall(r"(\w+);", body.replace("R, T;", "R; T;"))
        assert fields == [f[0] for f in struct._fields_], (name, fields)
    assert C.sizeof(L.cpmppi_dense_model) == 10 * 8 and C.sizeof(L.cpmppi_dense_control_args) == 8 + 6 * 8
    assert C.sizeof(L.cpmppi_dense_loss_args) == 5 * 4 + 4 + 8 * 8


def test_the_unit_is_built_and_documented():
    import __graft_entry__ as G
    assert "cpmppi_dense.hip" in G.HIP_UNITS
    from cartpolesimulation_amd import controller_neural_imitator, train_imitator
    assert "THIS PACKAGE'S OWN" in train_imitator.__doc__ and "SI_Toolkit" in train_imitator.__doc__
    assert "does not carry" in controller_neural_imitator.__doc__
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as fh:
            assert "train_imitator" in fh.read(), doc


def test_kernels_have_no_scratch_and_no_vgpr_spills():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    if not os.path.exists(os.path.join(code_objects.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    from cartpolesimulation_amd import _lib
    ks = [k for k in code_objects.kernels(_lib.LIB_PATH) if re.search(r"dense_(control|grad|finalize)_kernel", k["name"])]
    assert len(ks) == 4, [k["name"] for k in ks]                    # control, the forward with and without the gradient, finalize
    bad = [(k["name"], k["private_segment_fixed_size"], k["vgpr_spill_count"]) for k in ks
           if k["private_segment_fixed_size"] != 0 or k["vgpr_spill_count"] != 0]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 4. the reference
def network_c_loop(model, x):
    """One sample through the network the way C_implementation/network.c walks it: layer by layer, unit by unit, the sum over the
    inputs in index order starting from the bias, tanh on the hidden layers, nothing on the head (float64 throughout)."""
    a = np.asarray(model.get("in_scale", np.ones(7)), np.float64)
    b = np.asarray(model.get("in_shift", np.zeros(7)), np.float64)
    act = [float(a[k]) * float(x[k]) + float(b[k]) for k in range(7)]
    for wk, bk, last in (("w1", "b1", False), ("w2", "b2", False), ("w3", "b3", True)):
        w, bias = np.asarray(model[wk], np.float64), np.asarray(model[bk], np.float64)
        out = []
        for i in range(w.shape[0]):
            z = float(bias[i])
            for k in range(w.shape[1]):
                z += float(w[i, k]) * act[k]
            out.append(z if last else float(np.tanh(z)))
        act = out
    return act[0]


def test_reference_reproduces_the_network_c_loop_on_the_golden_weights():
    model = D.golden_model()
    s, tp, te, _ = D.recordings(11, R=1, T=24)
    q, y, raw = D.control(model, s[0], tp[0], te[0])
    x = D.features(s[0], tp[0], te[0]).astype(np.float64)
    want = np.array([network_c_loop(model, x[i]) for i in range(24)])
    assert np.abs(y - want).max() < 1e-13
    assert np.array_equal(q, np.clip(raw, -1.0, 1.0)) and np.abs(raw - want).max() < 1e-13      # (A = 1, B = 0 in the golden folder)


def test_reference_gradient_equals_central_differences():
    model = D.random_model(2, scale=0.5, norm=True)
    s, tp, te, lab = D.recordings(4, R=2, T=30)
    w = np.array([[0, 0], [1, 9], [1, 19]])
    x, y = D.samples(s, tp, te, lab, w, 10, 1)
    assert x.shape == (30, 7) and np.array_equal(y[:10], lab[0, 1:11]) and np.array_equal(x[10, 0:5], s[1, 9, 1:6])
    _, g = D.loss_and_grad(model, x, y)

    def loss64(flat):
        m = {k: torch.as_tensor(v) for k, v in zip(D.KEYS, np.split(flat, np.cumsum([int(np.prod(sh)) for sh in D.SHAPES])[:-1]))}
        m = {k: v.reshape(sh) for (k, v), sh in zip(m.items(), D.SHAPES)}
        a, b, A, B = D._norm(model, torch.float64)
        out = D.forward(m, torch.as_tensor(x).double() * a + b)
        return float(((out - (torch.as_tensor(y).double() - B) / A) ** 2).mean())

    flat = D.flatten(model).astype(np.float64)
    for p in (0, 100, 224, 300, 1000, 1290, 1320, 1344):
        h = np.zeros(D.NPAR)
        h[p] = 1e-6
        fd = (loss64(flat + h) - loss64(flat - h)) / 2e-6
        assert abs(fd - g[p]) <= 1e-6 * abs(g[p]) + 1e-10, (p, fd, g[p])


def test_reference_adam_is_the_headers_update():
    opt = D.Adam(np.zeros(D.NPAR, f32), 1e-3)
    g = np.linspace(-1, 1, D.NPAR)
    p1 = opt.step(g).copy()
    nz = np.abs(g) > 1e-3
    assert np.allclose(p1[nz], -1e-3 * np.sign(g[nz]), rtol=1e-4)   # the first bias-corrected step is lr * sign(g)
    assert p1[np.argmin(np.abs(g))] == 0.0 and opt.t == 1
    assert opt.m.dtype == np.float32 and np.allclose(opt.m, 0.1 * g, rtol=1e-6)
