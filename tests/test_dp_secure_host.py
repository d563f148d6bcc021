"""The secure DP noise without a GPU: the library's host ChaCha20
(sa_chacha20_blocks_host, the block function the kernels compile) against the
numpy restatement and the known answers, the sa_dp_secure mirror's layout,
the argument checks of the new entries, and SecureGaussianModelDP's
constructor logic."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import chacha_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_A, KEY_B, NONCE = bytes(range(32)), bytes(range(1, 33)), 7


def test_host_blocks_equal_the_known_answers(golden_dir):
    from sfl_amd import _lib as L

    with open(os.path.join(golden_dir, "chacha20_kat.json")) as f:
        kat = json.load(f)
    for e in kat:
        got = L.chacha20_blocks_host(bytes.fromhex(e["key"]), int(e["nonce"], 16), int(e["block"], 16), 1)
        assert [f"{int(w):08x}" for w in got[0]] == e["words"], (e["source"], e["block"])


@pytest.mark.parametrize("key,nonce,b0,nb", [
    (KEY_A, NONCE, 0, 1), (KEY_A, NONCE, 0, 257), (KEY_B, NONCE, 11, 64),
    (KEY_A, NONCE, (1 << 32) - 2, 5),  # blocks 2^32 - 2 .. 2^32 + 2: the carry into word 13
    (KEY_A, (1 << 64) - 1, (1 << 40) + 5, 9), (KEY_B, 1 << 32, (1 << 64) - 2, 4),  # wraps mod 2^64
])
def test_host_blocks_equal_the_restatement(key, nonce, b0, nb):
    from sfl_amd import _lib as L

    got = L.chacha20_blocks_host(key, nonce, b0, nb)
    assert got.shape == (nb, 16) and got.dtype == np.uint32
    assert np.array_equal(got, co.blocks(co.key_words(key), nonce, b0, nb))
    last = (b0 + nb - 1) & co.M64
    assert np.array_equal(got[-1], L.chacha20_blocks_host(key, nonce, last, 1)[0])
    if last >> 32:  # word 13 matters: a counter cut to 32 bits gives another block
        assert not np.array_equal(got[-1], L.chacha20_blocks_host(key, nonce, last & 0xFFFFFFFF, 1)[0])


def test_new_entries_validate_before_touching_the_gpu():
    from sfl_amd import _lib as L

    lib = L.lib()
    key = L.chacha_key_words(KEY_A)
    out = (C.c_uint32 * 16)()
    dp = L.DPSecure()
    calls = {
        "sa_chacha20_blocks_host (no key)": lambda: lib.sa_chacha20_blocks_host(None, 0, 0, 1, out),
        "sa_chacha20_blocks_host (no out)": lambda: lib.sa_chacha20_blocks_host(key, 0, 0, 1, None),
        "sa_chacha20_keystream (no out)": lambda: lib.sa_chacha20_keystream(key, 0, 0, 1, None, None),
        "sa_chacha20_keystream (no key)": lambda: lib.sa_chacha20_keystream(None, 0, 0, 1, 16, None),
        "sa_chacha20_keystream (out at +4)": lambda: lib.sa_chacha20_keystream(key, 0, 0, 1, 4100, None),
        "sa_hb_normals_f64": lambda: lib.sa_hb_normals_f64(None, 4, 1.0, None, None),
        "sa_dp_perturb_secure_f32 (no dp)": lambda: lib.sa_dp_perturb_secure_f32(None, 0, None, None, None),
        "sa_dp_perturb_secure_f32 (no x)": lambda: lib.sa_dp_perturb_secure_f32(None, 10, C.byref(dp), None, None),
        "sa_dp_perturb_secure_f32 (no sumsq)": lambda: lib.sa_dp_perturb_secure_f32(4096, 10, C.byref(dp), 8192, None),
    }
    for name, call in calls.items():
        assert call() == L.SA_ERR_ARG, name
        assert name.split(" ")[0].encode() in lib.sa_last_error(), name
    assert lib.sa_chacha20_blocks_host(key, 0, 0, 0, None) == L.SA_OK
    assert lib.sa_chacha20_keystream(key, 0, 0, 0, None, None) == L.SA_OK
    assert lib.sa_hb_normals_f64(None, 0, 1.0, None, None) == L.SA_OK
    with pytest.raises(ValueError):
        L.chacha_key_words(bytes(31))
    assert list(L.chacha_key_words(KEY_A))[:2] == [0x03020100, 0x07060504]


def test_dp_secure_mirror_matches_the_header_layout(tmp_path):
    """sfl_amd._lib.DPSecure has the C layout of sa_dp_secure (gcc's sizes
    and offsets): a stale mirror would pass the wrong key bytes silently."""
    from sfl_amd import _lib as L

    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = ["sumsq", "sumsq_layer", "l2_norm_clip", "noise_std", "num_updates", "key", "nonce", "counter0"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "sfl_sa.h")}"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(sa_dp_secure));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sa_dp_secure, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c11", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.DPSecure)
    for f in fields:
        assert int(got[f]) == getattr(L.DPSecure, f).offset, f


def test_secure_gaussian_model_dp_without_gpu():
    from sfl_amd.security.privacy import DPStrategyFL, GaussianModelDP, SecureGaussianModelDP

    a = SecureGaussianModelDP(noise_multiplier=1.0, num_clients=4)
    b = SecureGaussianModelDP(noise_multiplier=1.0, num_clients=4)
    assert isinstance(a, GaussianModelDP) and a.is_secure_generator is True
    assert isinstance(a.key, bytes) and len(a.key) == 32 and 0 <= a.nonce < 1 << 64
    assert (a.key, a.nonce) != (b.key, b.nonce)  # two unseeded instances differ
    assert a.counter == 0 and a.num_updates == 4 and a.delta == min(1 / 16, 1e-5)
    c = SecureGaussianModelDP(0.5, 8, num_updates=3, l2_norm_clip=2.0, is_clip_each_layer=True, key=KEY_A,
                              nonce=NONCE)
    assert (c.key, c.nonce, c.num_updates, c.is_clip_each_layer) == (KEY_A, NONCE, 3, True)
    assert c.noise_std == 0.5 * 2.0 * 2.0
    for bad in (bytes(31), bytes(33), b""):
        with pytest.raises(ValueError):
            SecureGaussianModelDP(1.0, 4, key=bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            SecureGaussianModelDP(1.0, 4, nonce=bad)
    with pytest.raises(TypeError):  # the reference's flag is not an argument here
        SecureGaussianModelDP(1.0, 4, is_secure_generator=True)
    with pytest.raises(TypeError, match="sa_mask_dp draws Philox noise"):
        c.params(None, 16)
    assert c.counter == 0
    with pytest.raises(NotImplementedError, match="SecureGaussianModelDP"):  # the base class still refuses the flag
        GaussianModelDP(noise_multiplier=1.0, num_clients=4, is_secure_generator=True)
    assert DPStrategyFL(model_gdp=c).model_gdp is c


def test_counter_rounds_up_to_whole_blocks(monkeypatch):
    """_perturb advances the counter by ceil(n / 4) * 4 per layer and hands
    the kernel the counter before the layer (kernels stubbed: no GPU)."""
    from sfl_amd import kernels as K
    from sfl_amd.security.privacy import SecureGaussianModelDP

    seen = []
    monkeypatch.setattr(K, "make_dp_secure", lambda sumsq, **kw: seen.append(kw) or kw)
    monkeypatch.setattr(K, "dp_perturb_secure", lambda x, y, dp: y)

    class Flat:
        def __init__(self, n):
            self.n = n

        def numel(self):
            return self.n

    m = SecureGaussianModelDP(1.0, 4, key=KEY_B, nonce=NONCE)
    for n in (5, 0, 8, 1):
        m._perturb(Flat(n), None, None, None)
    assert [kw["counter0"] for kw in seen] == [0, 8, 8, 16] and m.counter == 20
    assert all(kw["key"] == KEY_B and kw["nonce"] == NONCE and kw["noise_std"] == 1.0 for kw in seen)
