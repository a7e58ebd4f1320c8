"""The learner's two entry points at the C boundary, without a GPU: both are
exported and bound, and null or misaligned arguments come back as BGX_E_ARG
before any device (or the engine) is touched."""
import ctypes
import subprocess

from test_abi import built  # noqa: F401  (module fixture: builds libbgx.so when missing)

NAMES = ("bgx_set_weights_device", "bgx_episode_offsets")


def test_learner_symbols_are_exported_and_bound(built):  # noqa: F811
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in out, name
    from bgx._lib import SIGNATURES
    import bgx
    L = bgx.lib()
    for name in NAMES:
        assert name in SIGNATURES and getattr(L, name).restype is ctypes.c_int
    assert L.bgx_abi_version() == 10   # entry points were only added


def test_set_weights_device_argument_errors(built):  # noqa: F811
    import bgx
    L = bgx.lib()
    params = (ctypes.c_float * 25604)()
    p = ctypes.addressof(params)
    assert L.bgx_set_weights_device(None, p, 1.5, 1, None) == -1
    assert b"bgx_set_weights_device" in L.bgx_last_error() and b"engine" in L.bgx_last_error()
    # the argument checks come before the engine is read: any non-null handle will do here
    fake = (ctypes.c_uint8 * 64)()
    e = ctypes.addressof(fake)
    assert L.bgx_set_weights_device(e, None, 1.5, 1, None) == -1
    assert b"d_params" in L.bgx_last_error()
    for off in (1, 2, 3):
        assert L.bgx_set_weights_device(e, p + off, 1.5, 1, None) == -1
        assert b"aligned" in L.bgx_last_error()
    for t in (0.0, -1.0, float("nan")):
        assert L.bgx_set_weights_device(e, p, t, 1, None) == -1
        assert b"temperature" in L.bgx_last_error()
    assert bytes(fake) == bytes(64)


def test_episode_offsets_argument_errors(built):  # noqa: F811
    import bgx
    L = bgx.lib()
    hdr = (ctypes.c_uint32 * 64)()
    offs = (ctypes.c_int32 * 8)(*([77] * 8))
    h, o = ctypes.addressof(hdr), ctypes.addressof(offs)
    assert L.bgx_episode_offsets(h, -1, o, None) == -1
    assert b"bgx_episode_offsets" in L.bgx_last_error() and b"n_eps=-1" in L.bgx_last_error()
    assert L.bgx_episode_offsets(h, 2, None, None) == -1       # nowhere to write
    assert L.bgx_episode_offsets(None, 0, None, None) == -1    # ... even with no episodes (offs[0] is written)
    assert L.bgx_episode_offsets(None, 2, o, None) == -1       # headers to read, none given
    for off in (1, 2, 3):
        assert L.bgx_episode_offsets(h + off, 2, o, None) == -1
        assert b"aligned" in L.bgx_last_error()
        assert L.bgx_episode_offsets(h, 2, o + off, None) == -1
        assert b"aligned" in L.bgx_last_error()
    assert list(offs) == [77] * 8


def test_learner_python_surface():
    import bgx
    from bgx import learner, ops
    from bgx.engine import Engine
    from bgx.trainer import DeviceTrainer
    assert bgx.learner is learner and callable(learner.Learner) and callable(learner.reference_temperature)
    assert callable(ops.episode_offsets) and callable(Engine.set_weights_device)
    assert Engine.PEEK["net_frag"][0] == 9
    for name in ("update_device", "metrics", "sync_module", "state_dict", "publish"):
        assert callable(getattr(DeviceTrainer, name))
    # the reference schedule (parameter_manager.py get_temperature)
    t = learner.reference_temperature
    assert t(1) == 1.5 and t(4001) == 0.5 and t(10 ** 6) == 0.5 and abs(t(2001) - 1.0) < 1e-12
