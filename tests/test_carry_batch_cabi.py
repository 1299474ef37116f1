"""CPU checks of gamdp_carry_batch (the whole result from a fill alone, include/gamdp.h): the library exports it, its launch records
have the layout of gamdp_score_batch's, and the argument checks need no GPU."""
import ctypes

from gam_ngs_amd import lib


def test_carry_batch_is_exported():
    l = lib.load_library()
    for name in ("gamdp_carry_batch", "gamdp_ctx_carry_info"):
        assert name in lib.SYMBOLS
        assert hasattr(l, name)
    assert l.gamdp_carry_batch.argtypes[-1] == ctypes.POINTER(lib.Result)            # a gamdp_result per call, as gamdp_align_batch
    assert l.gamdp_ctx_carry_info.argtypes[1] == ctypes.POINTER(lib.ScoreLaunchInfo)


def test_null_arguments_are_einval():
    l = lib.load_library()
    out = (lib.Result * 1)()
    tasks = (lib.Task * 1)()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))   # never dereferenced: the NULL checks come first
    assert l.gamdp_carry_batch(None, None, None, None, 0, None) == lib.EINVAL
    assert l.gamdp_carry_batch(None, fake, fake, tasks, 1, out) == lib.EINVAL       # ctx
    assert l.gamdp_carry_batch(fake, None, fake, tasks, 1, out) == lib.EINVAL       # set_a
    assert l.gamdp_carry_batch(fake, fake, None, tasks, 1, out) == lib.EINVAL       # set_b
    assert l.gamdp_carry_batch(fake, fake, fake, tasks, 1, None) == lib.EINVAL      # out
    assert l.gamdp_carry_batch(fake, fake, fake, tasks, 0, None) == lib.EINVAL      # out, whatever n
    assert l.gamdp_carry_batch(fake, fake, fake, None, 1, out) == lib.EINVAL        # tasks with n > 0
    assert l.gamdp_ctx_carry_info(None, None, 0, None) == lib.EINVAL


def test_the_python_api_has_the_call():
    from gam_ngs_amd import api
    assert callable(api.BandedSmithWaterman.find_results) and callable(api.Context.carry_info)
