"""bj_verify_kernel_ms and bj_verify_batch_ms (csrc/verifier.hip): which call each one reports on, when each refuses, and that
neither disturbs the other's state.  One context of its own, so that no other test's verify decides what the calls answer; the
cases run in order on it."""
import numpy as np
import pytest

import era_boojum_amd as E
from era_boojum_amd import binding as B, synthetic as S
from gpu_util import ctx

pytestmark = pytest.mark.gpu


def _refused(call, cx):
    with pytest.raises(E.BoojumHipError):
        call(cx)


def test_kernel_ms_and_batch_ms_report_on_their_own_call():
    ctx()                                   # the session's context first: it settles which HIP runtime the process uses
    cx = E.Context(0)
    c = S.sha_shaped_circuit(9, seed=11, table_bits=2)
    s = E.ProverSetup(cx, c, 8, 16, 20)
    vk = s.verifier()
    try:
        buf, _ = s.prove()
        assert int(buf[9]) == 7
        # 1. nothing has run on this context
        _refused(vk.kernel_ms, cx)
        _refused(vk.batch_ms, cx)
        # 2. a verify that reaches its kernels
        assert vk.verify(cx, buf).stage == B.VERIFY_OK
        a, b = vk.kernel_ms(cx)
        assert a > 0 and b > 0
        _refused(vk.batch_ms, cx)
        # 3. a verify that ends on the host: the last bj_verify did not reach its kernels
        assert vk.verify(cx, buf[:-1]).stage == B.VERIFY_SHAPE
        _refused(vk.kernel_ms, cx)
        # 4. a batch of one answers for the batch alone
        assert vk.verify_batch(cx, [buf])[0].stage == B.VERIFY_OK
        host_ms, upload_ms, open_ms, deep_ms = vk.batch_ms(cx)
        assert open_ms > 0 and deep_ms > 0
        _refused(vk.kernel_ms, cx)
        # 5. both answer; a batch that ends on the host zeroes its own device phases and leaves bj_verify's figures alone
        assert vk.verify(cx, buf).stage == B.VERIFY_OK
        single = vk.kernel_ms(cx)
        assert single[0] > 0 and single[1] > 0
        assert vk.batch_ms(cx)[2] > 0 and vk.batch_ms(cx)[3] > 0
        magic = np.array(buf, copy=True)
        magic[0] += np.uint64(1)
        got = vk.verify_batch(cx, [buf[:-1], magic])
        assert [r.stage for r in got] == [B.VERIFY_SHAPE, B.VERIFY_SHAPE]
        host_ms, upload_ms, open_ms, deep_ms = vk.batch_ms(cx)
        assert host_ms > 0 and (upload_ms, open_ms, deep_ms) == (0.0, 0.0, 0.0)
        assert vk.kernel_ms(cx) == single
    finally:
        vk.close()
        s.close()
        cx.close()
