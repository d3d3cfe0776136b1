"""Model-folder reader (CPU): the reference's in-tree folder as format fixture, and a synthetic GRU folder round trip."""
import os

import numpy as np
import pytest

from cartpolesimulation_amd import model_folder as MF

f32 = np.float32

HERE = os.path.dirname(os.path.abspath(__file__))
DENSE = os.path.join(HERE, "golden", "model_folder", "Dense-7IN-32H1-32H2-1OUT-0")


def test_reads_the_reference_net_info_and_normalization():
    info = MF.read_net_info(DENSE)
    assert info["inputs"] == ["angleD", "angle_cos", "angle_sin", "position", "positionD", "target_equilibrium", "target_position"]
    assert info["outputs"] == ["Q_calculated_offline"]
    assert info["net_name"] == "Dense-32H1-32H2" and info["net_full_name"] == "Dense-7IN-32H1-32H2-1OUT-0"
    assert info["type"] == "Dense" and info["library"] == "TF" and info["normalize"] == "True"
    nm = MF.read_normalization(DENSE, info)
    np.testing.assert_allclose(nm["a"], [0.05440483, 1, 1, 5.05050516, 0.88866770, 1, 5.05050516], rtol=1e-7)
    assert not nm["b"].any() and nm["A"].tolist() == [1.0] and nm["B"].tolist() == [0.0]
    with pytest.raises(NotImplementedError):
        MF.load_gru_model(DENSE)                       # a Dense controller net is not the GRU predictor


def _write_gru_folder(root, inputs, outputs, weights, a, b, A, B, name="GRU-6IN-32H1-32H2-5OUT-0"):
    d = os.path.join(root, name)
    os.makedirs(d)
    with open(os.path.join(d, name + ".txt"), "w") as f:
        f.write("CREATED:\n2024-01-01 at time 00:00:00\n\nLIBRARY:\nPytorch\n\nNET NAME:\nGRU-32H1-32H2\n\nNET FULL NAME:\n" + name +
                "\n\nINPUTS:\n" + ", ".join(inputs) + "\n\nOUTPUTS:\n" + ", ".join(outputs) + "\n\nTYPE:\nGRU\n\nNORMALIZE:\nTrue\n")
    for fn, v in (("normalization_vec_a.csv", a), ("normalization_vec_b.csv", b), ("denormalization_vec_A.csv", A),
                  ("denormalization_vec_B.csv", B)):
        np.savetxt(os.path.join(d, fn), np.asarray(v)[None], delimiter=",", fmt="%.8f")
    np.savez(os.path.join(d, "weights.npz"), **weights)
    return d


def test_gru_folder_round_trip_with_permuted_features(tmp_path):
    rng = np.random.Generator(np.random.SFC64(2))
    u = lambda *s: rng.uniform(-0.3, 0.3, s).astype(np.float32)  # noqa: E731
    kernel = dict(w_ih0=u(96, 6), w_hh0=u(96, 32), b_ih0=u(96), b_hh0=u(96), w_ih1=u(96, 32), w_hh1=u(96, 32), b_ih1=u(96),
                  b_hh1=u(96), w_out=u(5, 32), b_out=u(5))
    a, b = rng.uniform(0.5, 2, 6).astype(np.float32), u(6)
    A, B = rng.uniform(0.5, 2, 5).astype(np.float32), u(5)
    # the folder lists its features in another order than the kernel's
    pin, pout = [3, 0, 5, 1, 4, 2], [4, 2, 0, 1, 3]
    inputs, outputs = [MF.KERNEL_INPUTS[i] for i in pin], [MF.KERNEL_OUTPUTS[i] for i in pout]
    folder_w = dict(kernel)
    folder_w["w_ih0"] = kernel["w_ih0"][:, pin]
    folder_w["w_out"], folder_w["b_out"] = kernel["w_out"][pout], kernel["b_out"][pout]
    d = _write_gru_folder(str(tmp_path), inputs, outputs, folder_w, a[pin], b[pin], A[pout], B[pout])
    m = MF.load_gru_model(d)
    for k, v in kernel.items():
        np.testing.assert_array_equal(m[k], v, err_msg=k)
    np.testing.assert_allclose(m["in_scale"], a, rtol=1e-6)
    np.testing.assert_allclose(m["in_shift"], b, atol=1e-7)
    np.testing.assert_allclose(m["out_scale"], A, rtol=1e-6)
    np.testing.assert_allclose(m["out_shift"], B, atol=1e-7)


def test_torch_state_dict_and_tensorflow_only_folders(tmp_path):
    torch = pytest.importorskip("torch")
    gru = torch.nn.GRU(6, 32, num_layers=2, batch_first=True)
    head = torch.nn.Linear(32, 5)
    d = _write_gru_folder(str(tmp_path), MF.KERNEL_INPUTS, MF.KERNEL_OUTPUTS, {}, np.ones(6), np.zeros(6), np.ones(5), np.zeros(5))
    os.remove(os.path.join(d, "weights.npz"))
    sd = {("rnn." + k): v for k, v in gru.state_dict().items()}
    sd.update({("head." + k): v for k, v in head.state_dict().items()})
    torch.save(sd, os.path.join(d, "ckpt.pt"))
    m = MF.load_gru_model(d)
    np.testing.assert_array_equal(m["w_hh1"], gru.weight_hh_l1.detach().numpy())
    np.testing.assert_array_equal(m["w_out"], head.weight.detach().numpy())
    os.remove(os.path.join(d, "ckpt.pt"))
    open(os.path.join(d, "saved_model.pb"), "w").close()           # a container that is not read: refused by name
    with pytest.raises(NotImplementedError, match="TensorFlow"):
        MF.load_gru_model(d)


def _keras_gru_layer(x_seq, h, k, rk, b, u):
    """The Keras GRU cell exactly as Keras states it for reset_after=True (gate blocks z, r, h; x @ kernel):
    z = sigmoid(x Wz + bz_i + h Uz + bz_r); r likewise; hh = tanh(x Wh + bh_i + r * (h Uh + bh_r)); h' = z h + (1 - z) hh."""
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))  # noqa: E731
    outs = []
    for x in x_seq:
        mx, mh = x @ k + b[0], h @ rk + b[1]
        z = sig(mx[:, :u] + mh[:, :u])
        r = sig(mx[:, u:2 * u] + mh[:, u:2 * u])
        hh = np.tanh(mx[:, 2 * u:] + r * mh[:, 2 * u:])
        h = z * h + (1.0 - z) * hh
        outs.append(h)
    return outs, h


def test_keras_weights_convert_to_the_torch_layout(tmp_path):
    """`model.get_weights()` of GRU(32) -> GRU(32) -> Dense(5) in the Keras layout (z, r, h gate blocks, x @ kernel,
    bias [2, 3u]) becomes, after keras_gru_weights_to_model, a torch.nn.GRU + Linear that computes the same sequence
    as the Keras equations evaluated directly on the Keras-layout arrays."""
    torch = pytest.importorskip("torch")
    rng = np.random.Generator(np.random.SFC64(8))
    u = 32
    g = lambda *s: (0.4 * rng.standard_normal(s)).astype(np.float64)  # noqa: E731
    arrays = [g(6, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 5), g(5)]
    model = MF.keras_gru_weights_to_model(arrays)
    B, T = 7, 9
    x = rng.standard_normal((T, B, 6))
    h0 = np.zeros((B, u)), np.zeros((B, u))
    o1, _ = _keras_gru_layer(list(x), h0[0], arrays[0], arrays[1], arrays[2], u)
    o2, _ = _keras_gru_layer(o1, h0[1], arrays[3], arrays[4], arrays[5], u)
    y_keras = np.stack(o2) @ arrays[6] + arrays[7]
    gru = torch.nn.GRU(6, u, num_layers=2).double()
    lin = torch.nn.Linear(u, 5).double()
    with torch.no_grad():
        for l in range(2):
            getattr(gru, f"weight_ih_l{l}").copy_(torch.as_tensor(model[f"w_ih{l}"], dtype=torch.float64))
            getattr(gru, f"weight_hh_l{l}").copy_(torch.as_tensor(model[f"w_hh{l}"], dtype=torch.float64))
            getattr(gru, f"bias_ih_l{l}").copy_(torch.as_tensor(model[f"b_ih{l}"], dtype=torch.float64))
            getattr(gru, f"bias_hh_l{l}").copy_(torch.as_tensor(model[f"b_hh{l}"], dtype=torch.float64))
        lin.weight.copy_(torch.as_tensor(model["w_out"], dtype=torch.float64))
        lin.bias.copy_(torch.as_tensor(model["b_out"], dtype=torch.float64))
        y_torch = lin(gru(torch.as_tensor(x))[0]).numpy()
    np.testing.assert_allclose(y_torch, y_keras, atol=2e-6)          # the arrays pass through float32 in the converter
    # the numpy GRU oracle (the checker the GPU kernel is held to) agrees with both on the converted dict
    from oracle import oracle_np as O
    m32 = {k: np.asarray(v, np.float32) for k, v in model.items()}
    h = np.zeros((2, B, u), np.float32)
    for t in range(T):
        h[0] = O.gru_cell(x[t].astype(np.float32), h[0], m32["w_ih0"], m32["w_hh0"], m32["b_ih0"], m32["b_hh0"])
        h[1] = O.gru_cell(h[0], h[1], m32["w_ih1"], m32["w_hh1"], m32["b_ih1"], m32["b_hh1"])
    np.testing.assert_allclose(h[1] @ m32["w_out"].T + m32["b_out"], y_keras[-1], atol=2e-5)
    # reset_after=False layers (bias [3u]) are a different cell
    bad = list(arrays)
    bad[2] = g(3 * u)
    with pytest.raises(NotImplementedError):
        MF.keras_gru_weights_to_model(bad)
    # a model folder that carries weights_keras.npz (the export INTEGRATION.md describes) loads through the same path
    d = _write_gru_folder(str(tmp_path), list(MF.KERNEL_INPUTS), list(MF.KERNEL_OUTPUTS), {}, np.ones(6), np.zeros(6),
                          np.ones(5), np.zeros(5))
    os.remove(os.path.join(d, "weights.npz"))
    np.savez(os.path.join(d, "weights_keras.npz"), *[a.astype(np.float32) for a in arrays])
    loaded = MF.load_gru_model(d)
    np.testing.assert_array_equal(loaded["w_hh1"], model["w_hh1"])


def test_predictor_output_augmentation_matches_the_reference():
    """predictors_customization.py:72-139, all three legs, against outputs of the reference's own class
    (tests/golden/augmentation.npz, oracle/gen_golden_augmentation.py)."""
    from types import SimpleNamespace
    from cartpolesimulation_amd.predictors import predictor_output_augmentation
    torch = pytest.importorskip("torch")
    g = np.load(os.path.join(HERE, "golden", "augmentation.npz"))
    for name in ("sincos", "angle_only", "angle_and_cos", "complete"):
        aug = predictor_output_augmentation(SimpleNamespace(outputs=[str(x) for x in g[f"{name}/outputs"]]))
        assert aug.get_indices_augmentation() == g[f"{name}/indices"].tolist()
        assert aug.get_features_augmentation() == [str(x) for x in g[f"{name}/features"]]
        np.testing.assert_allclose(aug.augment(g[f"{name}/x"]), g[f"{name}/y"], atol=1e-6)
        yt = aug.augment(torch.as_tensor(g[f"{name}/x"]))
        assert torch.is_tensor(yt)
        np.testing.assert_allclose(yt.numpy(), g[f"{name}/y"], atol=1e-6)
    diff = predictor_output_augmentation(SimpleNamespace(outputs=["D_angle_cos", "D_angle_sin", "D_position"]), differential_network=True)
    assert diff.get_features_augmentation() == ["angle"]


def test_conversion_is_pinned_to_keras():
    """tests/golden/keras_gru/{weights_keras.npz, keras_io.npz}: weights and outputs of a REAL Keras GRU(32) -> GRU(32) ->
    Dense(5), written by tools/export_keras_gru.py in a TensorFlow environment (none exists on this image, so the fixture
    may be absent: skipped then).  When present, the converted model must reproduce Keras' own outputs through
    torch.nn.GRU and through the numpy GRU oracle — the conversion is then pinned to Keras, not to the restatement of
    its equations above."""
    torch = pytest.importorskip("torch")
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keras_gru")
    if not (os.path.exists(os.path.join(d, "weights_keras.npz")) and os.path.exists(os.path.join(d, "keras_io.npz"))):
        pytest.skip("no Keras fixture: run tools/export_keras_gru.py once in a TensorFlow environment and commit tests/golden/keras_gru/")
    z = np.load(os.path.join(d, "weights_keras.npz"))
    io = np.load(os.path.join(d, "keras_io.npz"))
    model = MF.keras_gru_weights_to_model([z[f"arr_{i}"] for i in range(len(z.files))])
    x, y = io["x"].astype(np.float32), io["y"]
    gru = torch.nn.GRU(6, 32, num_layers=2, batch_first=True)
    head = torch.nn.Linear(32, 5)
    with torch.no_grad():
        for l in range(2):
            getattr(gru, f"weight_ih_l{l}").copy_(torch.tensor(model[f"w_ih{l}"]))
            getattr(gru, f"weight_hh_l{l}").copy_(torch.tensor(model[f"w_hh{l}"]))
            getattr(gru, f"bias_ih_l{l}").copy_(torch.tensor(model[f"b_ih{l}"]))
            getattr(gru, f"bias_hh_l{l}").copy_(torch.tensor(model[f"b_hh{l}"]))
        head.weight.copy_(torch.tensor(model["w_out"]))
        head.bias.copy_(torch.tensor(model["b_out"]))
        y_t = head(gru(torch.tensor(x))[0]).numpy()
    np.testing.assert_allclose(y_t, y, atol=2e-5, rtol=1e-5)


# ---- .keras archives (zip of config.json + model.weights.h5) read without TensorFlow / h5py ---------------------------
REF_KERAS = os.path.join(DENSE, "Dense-7IN-32H1-32H2-1OUT-0.keras")          # the reference folder's archive, stored verbatim


def test_hdf5_reader_round_trip():
    """cartpolesimulation_amd/hdf5_min.py against files written from the format specification by tests/hdf5_writer.py:
    nested groups, many children, float32 / float64 / float16 / int64 arrays, a scalar, an empty array."""
    from cartpolesimulation_amd.hdf5_min import read_hdf5
    from hdf5_writer import write_hdf5
    rng = np.random.Generator(np.random.SFC64(4))
    arrays = {"a/b/vars/0": rng.standard_normal((6, 96)).astype(np.float32),
              "a/b/vars/1": rng.standard_normal((32, 96)),
              "a/scalar": np.array(31260, np.int64),
              "a/half": rng.standard_normal(5).astype(np.float16),
              "top": np.arange(7, dtype=np.uint32),
              "empty/none": np.zeros((0, 3), np.float32)}
    arrays.update({f"many/child_{i:02d}": np.full((2, 2), i, np.float32) for i in range(20)})
    got = read_hdf5(write_hdf5(arrays))
    assert set(got) == set(arrays)
    for k, v in arrays.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), k
    with pytest.raises(ValueError, match="not an HDF5 file"):
        read_hdf5(b"PK\x03\x04" + b"\x00" * 64)


def _keras_archive(path, layers, arrays):
    import json
    import zipfile
    from hdf5_writer import write_hdf5
    config = {"module": "keras", "class_name": "Sequential", "config": {"name": "sequential", "layers": layers}}
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("metadata.json", json.dumps({"keras_version": "2.13.1"}))
        z.writestr("config.json", json.dumps(config))
        z.writestr("model.weights.h5", write_hdf5(arrays))


def test_model_folder_with_a_keras_archive_of_the_gru_predictor(tmp_path):
    """A GRU-6IN-32H1-32H2-5OUT folder whose weights exist only as <name>.keras — as SI_Toolkit saves them — loads: the
    archive's variables come out in model.get_weights() order (each GRU layer's kernel, recurrent kernel, bias from its
    cell; then the Dense head; optimizer slots and metrics ignored) and convert like an exported weights_keras.npz."""
    rng = np.random.Generator(np.random.SFC64(21))
    u = 32
    g = lambda *s: (0.3 * rng.standard_normal(s)).astype(f32)  # noqa: E731
    get_weights = [g(6, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 5), g(5)]
    top = "_layer_checkpoint_dependencies"
    arrays = {}
    for l, name in enumerate(("gru", "gru_1")):
        for i in range(3):
            arrays[f"{top}/{name}/cell/vars/{i}"] = get_weights[3 * l + i]
    arrays[f"{top}/dense/vars/0"], arrays[f"{top}/dense/vars/1"] = get_weights[6], get_weights[7]
    arrays["optimizer/vars/0"] = np.array(1000, np.int64)
    arrays["optimizer/vars/1"] = g(6, 3 * u)
    arrays["metrics/mean/vars/0"] = np.array(1.5, f32)
    layers = [{"class_name": "InputLayer", "config": {"name": "input_1", "batch_input_shape": [None, None, 6]}},
              {"class_name": "GRU", "config": {"name": "layers_0", "units": u}, "build_config": {"input_shape": [None, None, 6]}},
              {"class_name": "GRU", "config": {"name": "layers_1", "units": u}, "build_config": {"input_shape": [None, None, u]}},
              {"class_name": "Dense", "config": {"name": "layers_2", "units": 5}, "build_config": {"input_shape": [None, None, u]}}]
    d = _write_gru_folder(str(tmp_path), MF.KERNEL_INPUTS, MF.KERNEL_OUTPUTS, {}, np.ones(6), np.zeros(6), np.ones(5), np.zeros(5))
    os.remove(os.path.join(d, "weights.npz"))
    _keras_archive(os.path.join(d, os.path.basename(d) + ".keras"), layers, arrays)
    from cartpolesimulation_amd.hdf5_min import read_keras_weights
    got, owners = read_keras_weights(os.path.join(d, os.path.basename(d) + ".keras"))
    assert [c for _, c in owners] == ["GRU", "GRU", "Dense"] and len(got) == 8
    for a, b in zip(got, get_weights):
        assert np.array_equal(a, b)
    m = MF.load_gru_model(d)
    want = MF.keras_gru_weights_to_model(get_weights)
    for k in ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "w_out", "b_out"):
        np.testing.assert_array_equal(m[k], want[k])
    # a .keras archive of another architecture is refused by name, not mis-read
    layers[1]["class_name"] = "LSTM"
    arrays2 = {k.replace("/gru/", "/lstm/"): v for k, v in arrays.items()}
    _keras_archive(os.path.join(d, os.path.basename(d) + ".keras"), layers, arrays2)
    with pytest.raises(NotImplementedError, match="LSTM"):
        MF.load_gru_model(d)


def test_reference_keras_archive_equals_its_own_c_export(golden_dir):
    """The pin of the reader: the reference's in-tree model folder holds one trained network twice — as a .keras archive
    (written by Keras 2.13 / h5py) and as C arrays written by the reference's own export (C_implementation/
    network_parameters.c, parsed into tests/golden/keras_dense_c_export.npz by oracle/gen_golden_keras.py).  Read with
    hdf5_min.py, the archive reproduces the C export bit for bit."""
    from cartpolesimulation_amd.hdf5_min import read_keras_weights
    arrays, owners = read_keras_weights(REF_KERAS)
    assert [c for _, c in owners] == ["Dense", "Dense", "Dense"]
    gold = np.load(os.path.join(golden_dir, "keras_dense_c_export.npz"))
    for k in range(3):
        assert arrays[2 * k].dtype == np.float32
        assert np.array_equal(arrays[2 * k], gold[f"kernel{k}"]) and np.array_equal(arrays[2 * k + 1], gold[f"bias{k}"])


REF_CKPT = os.path.join(DENSE, "ckpt.ckpt")                                     # its TensorFlow checkpoint, stored verbatim


def test_reference_tf_checkpoint_equals_its_own_c_export(golden_dir):
    """The same pin for the other container: the in-tree folder's TensorFlow checkpoint (ckpt.ckpt.index + data shard,
    written by keras.Model.save_weights, Training.py:163), read with tf_bundle_min.py, reproduces the reference's C export
    of the network bit for bit; optimizer slots and the object graph are skipped."""
    from cartpolesimulation_amd.tf_bundle_min import read_keras_checkpoint_weights, read_tf_checkpoint
    arrays = read_keras_checkpoint_weights(REF_CKPT)
    gold = np.load(os.path.join(golden_dir, "keras_dense_c_export.npz"))
    assert len(arrays) == 6
    for k in range(3):
        assert np.array_equal(arrays[2 * k], gold[f"kernel{k}"]) and np.array_equal(arrays[2 * k + 1], gold[f"bias{k}"])
    names = read_tf_checkpoint(REF_CKPT)
    assert names["optimizer/_iterations/.ATTRIBUTES/VARIABLE_VALUE"].dtype == np.int64


def test_model_folder_with_only_a_tf_checkpoint(tmp_path):
    """A GRU-6IN-32H1-32H2-5OUT folder whose weights exist only as ckpt.ckpt.index + ckpt.ckpt.data-00000-of-00001 (written
    here from the format descriptions by tests/tf_bundle_writer.py, several table blocks, prefix-compressed keys) loads
    and converts like model.get_weights()."""
    from tf_bundle_writer import write_tf_checkpoint
    from cartpolesimulation_amd.tf_bundle_min import read_tf_checkpoint
    rng = np.random.Generator(np.random.SFC64(22))
    u = 32
    g = lambda *s: (0.3 * rng.standard_normal(s)).astype(f32)  # noqa: E731
    get_weights = [g(6, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 3 * u), g(u, 3 * u), g(2, 3 * u), g(u, 5), g(5)]
    t = {}
    for l in range(2):
        for i, kind in enumerate(("kernel", "recurrent_kernel", "bias")):
            t[f"layer_with_weights-{l}/cell/{kind}/.ATTRIBUTES/VARIABLE_VALUE"] = get_weights[3 * l + i]
    t["layer_with_weights-2/kernel/.ATTRIBUTES/VARIABLE_VALUE"] = get_weights[6]
    t["layer_with_weights-2/bias/.ATTRIBUTES/VARIABLE_VALUE"] = get_weights[7]
    t["optimizer/_iterations/.ATTRIBUTES/VARIABLE_VALUE"] = np.array(77, np.int64)
    t["optimizer/_variables/1/.ATTRIBUTES/VARIABLE_VALUE"] = g(6, 3 * u)
    d = _write_gru_folder(str(tmp_path), MF.KERNEL_INPUTS, MF.KERNEL_OUTPUTS, {}, np.ones(6), np.zeros(6), np.ones(5), np.zeros(5))
    os.remove(os.path.join(d, "weights.npz"))
    write_tf_checkpoint(os.path.join(d, "ckpt.ckpt"), t)
    back = read_tf_checkpoint(os.path.join(d, "ckpt.ckpt"))
    assert set(back) == set(t) and all(np.array_equal(back[k], t[k]) and back[k].dtype == t[k].dtype for k in t)
    m = MF.load_gru_model(d)
    want = MF.keras_gru_weights_to_model(get_weights)
    for k in want:
        np.testing.assert_array_equal(m[k], want[k])
