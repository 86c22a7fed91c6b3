"""Host-side decisions of the dgv2_gemm_stream_* entries (gemm_stream.hip): argument checks and the geometries they hand
back to the generic engines.  All of them are taken before anything touches the device, so they can be held without one;
the pointers are never dereferenced on these paths."""
import dgv2_native as N

P16, ODD = 1 << 20, (1 << 20) + 8   # a 16-byte aligned and a misaligned non-null address
EINVAL = -1


def nn(y=P16, x=P16, w=P16, B=2, P=128, I=64, O=128, ldx=None, ldy=None, wstride=None, resid=None, act=0, dt=N.BF16, ydt=N.BF16):
    return N.lib.dgv2_gemm_stream_nn(y, x, w, B, P, I, O, I if ldx is None else ldx, O if ldy is None else ldy,
                                     O * I if wstride is None else wstride, None, None, act, 0.2, 1.0, resid, dt, ydt, None, 0,
                                     None, None)


def nn_cat(y=P16, xa=P16, xs=P16, w=P16, B=2, P=128, Ka=32, Ks=64, O=128, act=0, dt=N.BF16, ydt=N.BF16):
    return N.lib.dgv2_gemm_stream_nn_cat(y, xa, xs, w, B, P, Ka, Ks, O, None, None, act, 0.2, 1.0, dt, ydt, None, 0, None, None)


def tn(gw=P16, gy=P16, x=P16, B=2, P=128, I=128, O=64, ldgy=None, ldx=None, dt=N.BF16):
    return N.lib.dgv2_gemm_stream_tn(gw, gy, x, B, P, I, O, O if ldgy is None else ldgy, I if ldx is None else ldx, dt, None)


def tn_cat(gw=P16, gy=P16, xa=P16, xs=P16, B=2, P=128, Ka=64, Ks=64, O=64, dt=N.BF16):
    return N.lib.dgv2_gemm_stream_tn_cat(gw, gy, xa, xs, B, P, Ka, Ks, O, dt, None)


def test_invalid_arguments():
    """What the generic entries call invalid is invalid here too (not a request for the fallback)."""
    assert nn(y=None) == EINVAL and nn(x=None) == EINVAL and nn(w=None) == EINVAL
    assert nn(B=0) == EINVAL and nn(P=0) == EINVAL and nn(I=0) == EINVAL and nn(O=0) == EINVAL
    assert nn(ldx=32) == EINVAL and nn(ldy=64) == EINVAL and nn(act=1) == EINVAL
    assert nn_cat(y=None) == EINVAL and nn_cat(xs=None) == EINVAL and nn_cat(w=None) == EINVAL and nn_cat(xa=None) == EINVAL
    assert nn_cat(B=0) == EINVAL and nn_cat(Ka=-8) == EINVAL and nn_cat(Ks=0) == EINVAL and nn_cat(act=2) == EINVAL
    assert nn_cat(Ka=4) == EINVAL and nn_cat(Ks=60) == EINVAL                    # off the 16-byte chunk
    assert nn_cat(xs=ODD) == EINVAL and nn_cat(xa=ODD) == EINVAL and nn_cat(w=ODD) == EINVAL and nn_cat(y=ODD) == EINVAL
    assert tn(gw=None) == EINVAL and tn(gy=None) == EINVAL and tn(x=None) == EINVAL
    assert tn(B=0) == EINVAL and tn(P=0) == EINVAL and tn(ldgy=32) == EINVAL and tn(ldx=64) == EINVAL
    assert tn_cat(gw=None) == EINVAL and tn_cat(xs=None) == EINVAL and tn_cat(xa=None) == EINVAL
    assert tn_cat(Ks=0) == EINVAL and tn_cat(Ka=4) == EINVAL and tn_cat(xs=ODD) == EINVAL and tn_cat(xa=ODD) == EINVAL


def test_nn_geometries_handed_back():
    assert nn(dt=N.F32, ydt=N.F32) == N.ENOTSUP                 # fp32 parity mode
    assert nn(ydt=N.F32) == N.ENOTSUP                           # fp32 output of bf16 operands (the heads)
    for O in (16, 32, 64):                                      # the generic TO = 16 / 32 / 64 instances
        assert nn(O=O) == N.ENOTSUP
    assert nn(I=48) == N.ENOTSUP and nn(I=8) == N.ENOTSUP       # K off the 32-grid
    assert nn(ldx=68) == N.ENOTSUP and nn(wstride=128 * 64 + 4) == N.ENOTSUP and nn(ldy=130) == N.ENOTSUP
    assert nn(y=ODD) == N.ENOTSUP and nn(x=ODD) == N.ENOTSUP and nn(w=ODD) == N.ENOTSUP and nn(resid=ODD) == N.ENOTSUP
    assert nn(P=1 << 23, I=256) == N.ENOTSUP                    # a sample's operand past 32-bit element offsets


def test_nn_cat_geometries_handed_back():
    assert nn_cat(dt=N.F32, ydt=N.F32) == N.ENOTSUP
    assert nn_cat(O=64) == N.ENOTSUP and nn_cat(O=16) == N.ENOTSUP
    assert nn_cat(Ka=0, Ks=40) == N.ENOTSUP                     # contraction off the 32-grid
    assert nn_cat(Ka=8, Ks=56) == N.ENOTSUP                     # the split inside a K-step
    assert nn_cat(O=130) == N.ENOTSUP


def test_tn_geometries_handed_back():
    assert tn(dt=N.F32) == N.ENOTSUP and tn_cat(dt=N.F32) == N.ENOTSUP
    assert tn(O=32) == N.ENOTSUP and tn(O=16) == N.ENOTSUP and tn_cat(O=32) == N.ENOTSUP
    assert tn(O=68) == N.ENOTSUP and tn(I=132) == N.ENOTSUP
    assert tn(B=1, P=1024) == N.ENOTSUP and tn_cat(B=1, P=1024) == N.ENOTSUP     # the generic entry splits K there
    assert tn(gw=ODD) == N.ENOTSUP and tn(gy=ODD) == N.ENOTSUP and tn(x=ODD) == N.ENOTSUP
    assert tn_cat(gw=ODD) == N.ENOTSUP and tn_cat(gy=ODD) == N.ENOTSUP
    assert tn(ldgy=68) == N.ENOTSUP and tn(ldx=132) == N.ENOTSUP
