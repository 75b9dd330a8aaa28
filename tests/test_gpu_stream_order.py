"""Every entry point keeps stream order with the caller's work (include/itw_amd.h: a device -> device call is asynchronous on the calling
thread's stream; a mixed call stages the host side on a stream of the library's and returns synchronised).  The library moves work onto
streams of its own under that promise -- two bands of BC7 `slow` with fork, mid and join events, the wide shape's second stream, every
mixed call on the thread's own stream behind a hipStreamSynchronize of the caller's, the workspace shared across streams through an
event -- and these tests are the ones that notice when one of those waits goes missing: the caller's stream is kept busy by a calibrated
delay while the library is called, with a witness that the delay was still running.  The sequences, the delay and the case table are in
tests/_stream_order.py; tests/test_stream_order_cases.py holds the table against the library's exported symbols.

Every test runs on a non-blocking side stream, after one warm-up call of the same arguments and a device synchronisation (growing the
workspace frees it, which waits for the device by design; the BC4 / BC5 tables are built on first use).

MEASURED on an MI355X (five runs of this module; the module prints the figures again at its end and, with ITW_STREAM_ORDER_REPORT=<file>,
writes them there):
  * the delay D: target 100 ms; calibrated to 121 .. 122 dependent mm(4096 x 4096, fp32), timed at 110.2 .. 110.8 ms.
  * largest host time from ev_ready.record() to the witness 0.017 ms, to the return of a call that did not wait 0.115 ms (the two-band
    BC7 `slow` call; 0.10 ms for a preview): D is about 900 times that, the rule asks for 10, so D stays at 100 ms.  Every witness was armed.
  * every sequence A call returned before the delay ended -- the capturable ones, which must, and the others too: itwDecodeChain and
    itwMeasureChain (descriptor table upload), itwGenerateMipChain on every route, itwGenerateMipChainAlpha with weight and coverage,
    itwPrepareNormalMapChain, itwQuantizeNormalMapChain, the device pad and converts, CompressImageMT with device pointers (which is one
    CompressBlocks* call on the calling thread, not a synchronous call: csrc/dispatch.hip).  This is recorded, not asserted.
  * sequence D on the library before compress_single_run and compress_runs waited for the caller's stream with a device destination: the two
    single-run cases (bc1, bc7 `basic`) failed -- the destination was overwritten under the reader; the two staged-runs cases passed, as
    did the sliced and chain ones.  The staged runs, the windows and the chain groups waited for the delay on that MI355X even in a build
    without WindowPipeline's synchronise (their first operation is a pageable upload on the thread's copy stream, which did not start
    before the caller's stream had drained; supposed: the runtime's few hardware queues are shared between streams), so a pass of those
    four routes shows no more than that; the single-run route, whose upload is on the thread's kernel stream, is the one that showed the
    race.  With the wait in both places all eight pass.
  * teeth, each in a scratch build: without WindowPipeline's synchronise 19 sequence B cases fail (all sliced, chain and mipped calls from
    device sources); without the wait in OrderedBuffer::claim the three sequence E tests fail; without the join of launch_rgb_bounded
    nothing failed -- the band on the second stream had ended by the time the caller's clone ran, the check is one-sided.
"""
import os

import pytest

import _stream_order as so
from conftest import first_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(itw, gpu, oracle):
    import torch
    itw.lib().itwWarmupBC45()
    itw.lib().itwWarmupBC45S()
    delay = so.Delay(torch, gpu)
    S = torch.cuda.Stream(gpu)
    delay(S)                                                      # the GEMM's first use of this stream
    torch.cuda.synchronize()
    e = so.Env(itw, oracle, gpu, torch, delay, S, so.Report())
    yield e
    for L in (itw.lib(), itw.test_lib()):
        L.itwSetStream(None)                                      # the thread's stream back to the default stream
        L.itwSetBc7Path(0)
    torch.cuda.synchronize()
    lines = e.report.lines(delay)
    print("\n" + "\n".join(lines))
    path = os.environ.get("ITW_STREAM_ORDER_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _cases(scheme):
    return [pytest.param(c, id=c.id) for c in so.CASES if c.scheme == scheme]


# ---- A. device -> device: read after write on the input, the consumer's view of the output, the join back ----------------------------------

@pytest.mark.parametrize("case", _cases("A"))
def test_a_device_call_is_in_stream_order(env, case):
    so.run_device(case.id, case.build(env), env, must_return_early=case.capturable)


# ---- B / C. synchronous calls with a device source --------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _cases("B"))
def test_b_synchronous_call_waits_for_the_producer_of_its_source(env, case):
    so.run_sync(case.id, case.build(env), env)


# ---- D. host source, device destination -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _cases("D"))
def test_d_host_source_call_waits_for_the_readers_of_its_destination(env, case):
    so.run_host_source(case.id, case.build(env), env)


# ---- E. the shared workspace across streams -----------------------------------------------------------------------------------------------

def _encode(env, fmt, prof, d_img, out):
    env.itw.compress(fmt, d_img, prof, out=out)


def _same_stream(env, fmt, got, want, what):
    m = first_mismatch(got.cpu().numpy(), want, 16)
    assert m is None, (what, m)


@pytest.mark.parametrize("second", [("bc6h", "slow", 64, 64), ("bc7", "slow", 64, 64)], ids=["bc7-then-bc6h", "bc7-then-bc7"])
def test_e_a_second_stream_claims_the_workspace_behind_the_first(env, second):
    """BC7 `slow` of 512 x 256 on stream P behind a delay, then at once a `slow` call on stream Q, which claims the thread's one workspace
    after P's call did: when Q's work has ended, P's has too (step 4) -- Q had to wait for the event that done() recorded behind P's use.
    That is the documented ordering of the shared workspace across streams (include/itw_amd.h, itwSetStream: "cross-stream ordering of its
    per-thread BC7 workspace uses library-owned events"); both outputs equal the oracle."""
    torch, itw = env.torch, env.itw
    fmt2, prof2, w2, h2 = second
    img1, img2 = so.texels("bc7", "slow", 512, 256, 1), so.texels(fmt2, prof2, w2, h2, 2)
    want1, want2 = so.encoded(env, "bc7", "slow", img1, (512, 256, 1)), so.encoded(env, fmt2, prof2, img2, (w2, h2, 2))
    d1, d2 = env.dev(img1), env.dev(img2)
    out1 = torch.empty(want1.size, dtype=torch.uint8, device=env.gpu)
    out2 = torch.empty(want2.size, dtype=torch.uint8, device=env.gpu)
    P, Q = env.S, torch.cuda.Stream(env.gpu)
    for timed in (False, True):
        out1.fill_(so.PRE)
        out2.fill_(so.PRE)
        torch.cuda.synchronize()
        with torch.cuda.stream(P):
            if timed:
                env.delay(P)
            _encode(env, "bc7", "slow", d1, out1)
            evP = torch.cuda.Event()
            evP.record(P)
        armed = not evP.query()
        with torch.cuda.stream(Q):
            _encode(env, fmt2, prof2, d2, out2)
            evQ = torch.cuda.Event()
            evQ.record(Q)
        evQ.synchronize()
        p_done = evP.query()
        torch.cuda.synchronize()
    assert armed, so.NOT_ARMED
    assert p_done, "the call on the second stream ended while the first stream's call still used the workspace"
    _same_stream(env, "bc7", out1, want1, "stream P")
    _same_stream(env, fmt2, out2, want2, "stream Q")
    assert itw.last_error() is None


def test_e_the_workspace_grows_under_a_call_in_flight_on_another_stream(env):
    """BC7 `basic` of 64 x 64 on P behind a delay; BC7 `slow` of 512 x 256 on Q needs a larger workspace, so it grows -- freeing the old one
    waits for the device, so the call on Q may block the host.  Both outputs equal the oracle."""
    torch, itw = env.torch, env.itw
    img1, img2 = so.texels("bc7", "basic", 64, 64, 1), so.texels("bc7", "slow", 512, 256, 1)
    want1, want2 = so.encoded(env, "bc7", "basic", img1, (64, 64, 1)), so.encoded(env, "bc7", "slow", img2, (512, 256, 1))
    d1, d2 = env.dev(img1), env.dev(img2)
    out1 = torch.full((want1.size,), so.PRE, dtype=torch.uint8, device=env.gpu)
    out2 = torch.full((want2.size,), so.PRE, dtype=torch.uint8, device=env.gpu)
    # a thread of its own has a workspace of its own, which has not grown yet
    import threading
    failure = []

    def body():
        try:
            torch.cuda.set_device(env.gpu)
            P, Q = torch.cuda.Stream(env.gpu), torch.cuda.Stream(env.gpu)
            with torch.cuda.stream(P):
                env.delay(P)
                _encode(env, "bc7", "basic", d1, out1)
                ev = torch.cuda.Event()
                ev.record(P)
            armed = not ev.query()
            with torch.cuda.stream(Q):
                _encode(env, "bc7", "slow", d2, out2)
            torch.cuda.synchronize()
            itw.lib().itwSetStream(None)
            assert armed, so.NOT_ARMED
            assert itw.last_error() is None, itw.last_error()
        except BaseException as e:                                # noqa: B036 -- reported on the test's thread
            failure.append(e)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failure:
        raise failure[0]
    _same_stream(env, "bc7", out1, want1, "stream P")
    _same_stream(env, "bc7", out2, want2, "stream Q")
