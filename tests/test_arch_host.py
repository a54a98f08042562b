"""CPU: architectures other than (embed_dim 64, n_heads 4) - the fixtures of tests/golden/arch_variants.npz
(tools/gen_golden_arch.py: the reference's own outputs), checkpoints of such models, and the supported set that
pf_create enforces before it touches a device."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pf_oracle as O
from phyloformer_amd.weights import random_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arch_weights(g, k):
    """Regenerate the weights of architecture k of arch_variants.npz; the blob hash must match the stored one."""
    E, H, nb = (int(v) for v in g["archs"][k])
    w = random_weights(int(g[f"a{k}/seed"]), n_blocks=nb, n_heads=H, embed_dim=E, scale=float(g["scale"]))
    assert hashlib.sha256(w.blob().tobytes()).hexdigest() == str(g[f"a{k}/sha"]), \
        f"random_weights no longer reproduces architecture {k}: the fixtures need regenerating"
    return w


def cases(g, k):
    c = 0
    while f"a{k}/idx{c}" in g.files:
        yield g[f"a{k}/idx{c}"], g[f"a{k}/out{c}"]
        c += 1


def test_oracle_matches_reference_on_every_architecture(golden):
    """fp32 and fp64 oracles against the reference's fp32 module on all six architectures (E = 40 has padded channels
    in the device path: the oracle has none, so this pins the fixtures themselves)."""
    g = golden("arch_variants.npz")
    assert len(g["archs"]) == 6
    for k in range(len(g["archs"])):
        w = arch_weights(g, k)
        n = 0
        for idx, want in cases(g, k):
            for dt in (np.float32, np.float64):
                got = O.forward(w.tensors, idx, n_blocks=w.n_blocks, n_heads=w.n_heads, dtype=dt).astype(np.float64)
                assert got.shape == want.shape
                assert float(np.abs(got - want).max()) <= 1e-4, (k, idx.shape, dt)
            n += 1
        assert n >= 3


def test_lightning_checkpoint_of_a_custom_architecture(tmp_path):
    """A Lightning-style .ckpt (model.-prefixed keys, conv-shaped tensors) of a (128, 8, 3) model is read with its
    architecture, by the torch-free reader and by the weights loader."""
    torch = pytest.importorskip("torch")
    from phyloformer_amd.ckpt import load_state_dict
    from phyloformer_amd.weights import load_weights
    w = random_weights(3, n_blocks=3, n_heads=8, embed_dim=128, scale=2.0)
    sd = {}
    for key, t in w.tensors.items():
        shape = t.shape
        if key.endswith("_proj.weight") or key.endswith("ffn.0.weight") or key.endswith("ffn.3.weight") \
                or key == "embedding_block.0.weight" or key == "pwFNN.0.weight":
            shape = t.reshape(t.shape[0] if t.ndim > 1 else 1, -1).shape + (1, 1)
        sd["model." + key] = torch.from_numpy(t.reshape(shape).copy())
    path = tmp_path / "custom.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": {"nb_blocks": 3, "embed_dim": 128, "nb_heads": 8}}, str(path))
    raw, _hp = load_state_dict(str(path))
    assert raw["embedding_block.0.weight"].shape[0] == 128
    lw = load_weights(str(path))
    assert (lw.n_blocks, lw.n_heads, lw.embed_dim) == (3, 8, 128)
    assert np.array_equal(lw.blob(), w.blob())


@pytest.mark.parametrize("E,H,nb,alphabet", [(30, 4, 1, 22), (320, 4, 1, 22), (64, 4, 1, 21), (64, 4, 65, 22)])
def test_unsupported_architectures_refused_before_device_access(E, H, nb, alphabet):
    """pf_create refuses what the generic kernels do not cover (embed_dim % n_heads != 0, embed_dim > 256, another
    alphabet, more than 64 blocks) with PF_EINVAL and the rule - before it looks for a device, so also without one."""
    from phyloformer_amd import engine
    lib = engine.load_library()
    wts = random_weights(0, n_blocks=nb, n_heads=H, embed_dim=E) if E % H == 0 and nb <= 2 else None
    n = lib.pf_blob_len(nb, H, E)
    blob = wts.blob() if wts is not None and wts.blob().size == n else np.zeros(n, np.float32)
    w = engine.pf_weights_t(nb, H, E, alphabet, blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size)
    h = C.c_void_p()
    rc = lib.pf_create(C.byref(w), 0, C.byref(h))
    assert rc == engine.PF_EINVAL and not h.value
    msg = lib.pf_last_error(None).decode()
    assert "embed_dim must be 1..256 and divisible by n_heads" in msg, msg
    if alphabet == 22 and nb == 1:
        with pytest.raises(ValueError, match="embed_dim must be 1..256 and divisible by n_heads"):
            engine.Engine(random_weights(0, n_blocks=nb, n_heads=H, embed_dim=E))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_blob_reader_follows_blob_layout(golden, tmp_path):
    """The C++ side's one reader of the checkpoint blob (csrc/pf_host_prep.h::read_blob) against
    weights.py::blob_layout: every field's offset in blob order and the total length, for the shipped (64, 4, 6) and the
    six architectures of arch_variants.npz (embed_dim 40 is no multiple of 16), and two with n_heads = embed_dim."""
    from phyloformer_amd.weights import blob_layout
    lib_path = str(tmp_path / "libpf_host_prep_shim.so")
    res = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                          os.path.join(REPO, "tests", "native", "pf_host_prep_shim.cpp"), "-o", lib_path],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    shim = C.CDLL(lib_path)
    shim.t_blob_offsets.restype = C.c_longlong
    shim.t_blob_offsets.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    archs = [(64, 4, 6), (16, 16, 1), (256, 256, 2)] + [tuple(int(v) for v in a) for a in golden("arch_variants.npz")["archs"]]
    assert any(E % 16 for E, _, _ in archs) and any(E == H for E, H, _ in archs)
    for E, H, nb in archs:
        sizes = [int(np.prod(shape)) for _, shape in blob_layout(nb, H, E)]
        want = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        blob = np.zeros(int(want[-1]), np.float32)
        got = np.full(len(sizes), -1, np.int64)
        n = shim.t_blob_offsets(blob.ctypes.data_as(C.POINTER(C.c_float)), nb, E, H,
                                got.ctypes.data_as(C.POINTER(C.c_longlong)))
        assert len(sizes) == 4 + 26 * nb
        assert n == want[-1], (E, H, nb)
        assert np.array_equal(got, want[:-1]), (E, H, nb)
