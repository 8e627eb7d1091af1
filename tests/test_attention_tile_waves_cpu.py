"""u3d_attn_tile_waves / precision.attn_tile_waves (include/u3d.h; csrc/attn_x3.hip "tile waves") is host state: no GPU needed."""
import pytest


def test_attn_tile_waves_switch_is_host_state():
    from unidet3d_amd import _lib
    l = _lib.lib()
    prev = l.u3d_attn_tile_waves(-1)
    try:
        assert prev in (0, 4, 8)
        assert l.u3d_attn_tile_waves(0) == prev and l.u3d_attn_tile_waves(-1) == 0
        last = 0
        for w in (4, 8, 4, 0):
            assert l.u3d_attn_tile_waves(w) == last          # returns the previous value ...
            assert l.u3d_attn_tile_waves(-1) == w            # ... and holds the new one
            last = w
        l.u3d_attn_tile_waves(8)
        for bad in (-1, 1, 2, 3, 5, 6, 7, 9, 16, 64, 128, -8):  # anything else only queries (6: no six-wave form is instantiated)
            assert l.u3d_attn_tile_waves(bad) == 8
        assert l.u3d_attn_tile_waves(-1) == 8
    finally:
        l.u3d_attn_tile_waves(prev)


def test_attn_tile_waves_context_manager_restores_and_refuses_other_values():
    from unidet3d_amd import _lib
    from unidet3d_amd import precision as P
    l = _lib.lib()
    prev = P.set_attn_tile_waves(0)
    try:
        with P.attn_tile_waves(8):
            assert l.u3d_attn_tile_waves(-1) == 8
            with P.attn_tile_waves(4):
                assert l.u3d_attn_tile_waves(-1) == 4
            assert l.u3d_attn_tile_waves(-1) == 8
        assert l.u3d_attn_tile_waves(-1) == 0
        for bad in (-1, 2, 5, 6, 16):
            with pytest.raises(ValueError):
                P.set_attn_tile_waves(bad)
        with pytest.raises(ValueError):
            with P.attn_tile_waves(7):
                pass
        assert l.u3d_attn_tile_waves(-1) == 0
    finally:
        P.set_attn_tile_waves(prev)
