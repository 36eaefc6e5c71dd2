"""The whole-picture faces on a caller's stream, as a decoder with frame threads runs them (INTEGRATION.md "Frame threads"):
streams made by ffhip_stream_create are hipStreamNonBlocking, so whatever a launcher leaves on the NULL stream (a memset of the
counters, the copy of the picture structs into a pool slot, the first kernel of a two-kernel call, a first-use table upload) is not
ordered against the caller's work at all.  Every other picture-face test runs on the NULL stream, where that cannot show.

test_face_on_a_created_stream   each of the 14 faces alone: poisoned tensors, then on one created stream a delay, the copies that put
                                the real inputs in place, the face, and a snapshot of its outputs; one ffhip_stream_synchronize.  A
                                face that runs any part of itself elsewhere reads poison or is snapshotted too early
                                (tests/test_picture_faces_cpu.py shows that both give a mismatch).
test_face_behind_a_busy_null_stream  each face again for foreign work that would run too late: dirtied pool slots, a busy NULL stream.
test_chains_on_a_created_stream the chained tests of the HEVC, VP9 and VP8 faces (their own set-up) the first way.
test_frame_threads              four threads, a stream and two pictures each, the codec's faces queued again and again with no
                                synchronisation: more slot-taking launches in flight than the progress pool has slots.
test_first_use_on_a_created_stream  a fresh process whose first call into the library is on a created stream."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import picture_faces as PF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
#: seconds: three times the slowest child measured on an MI355X machine (profiles/picture_streams_tests.txt: 2.1 .. 2.8 s, nearly all of
#: it the start of a fresh process with torch, and no slower when that start was the first on the machine), rounded up
CHILD_TIMEOUT = 9


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def delay():
    return PF.Delay(_torch())


@pytest.fixture
def stream():
    L = _lib()
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    yield st
    assert L.ffhip_stream_destroy(st) == 0


@pytest.mark.parametrize("name", PF.NAMES)
def test_face_on_a_created_stream(name, stream, delay):
    torch = _torch()
    face = PF.make(name)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [face], delay)
    PF.check_staged(torch, [face], view, ins)


@pytest.mark.parametrize("name", PF.NAMES)
def test_face_behind_a_busy_null_stream(name, stream, delay):
    """the same face when foreign work would run too late (run_staged, late=True): every pool slot holds a decoy's structs and spent
    counters, and the NULL stream is busy while the face runs on the created one"""
    torch = _torch()
    face = PF.make(name)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [face], delay, late=True)
    PF.check_staged(torch, [face], view, ins)


def _chains(codec):
    """the chained tests' own set-up (each file's Chain), as those tests run it on the NULL stream.  HEVC: the two chains that
    exist, residual -> inter -> intra -> loop filter and boundary strengths -> loop filter, one behind the other on the stream."""
    if codec == "hevc":
        import test_gpu_hevc_bs_picture as TB
        import test_gpu_hevc_res_picture as TR
        return [TR.Chain(10, 2), TB.Chain()]
    if codec == "vp9":
        import test_gpu_vp9_intra_frame as T9
        return [T9.Chain()]
    import test_gpu_vp8_recon as T8
    return [T8.Chain()]


@pytest.mark.parametrize("codec", PF.CODECS)
def test_chains_on_a_created_stream(codec, stream, delay):
    torch = _torch()
    chains = _chains(codec)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, chains, delay)
    PF.check_staged(torch, chains, view, ins)


#: per codec, how often a thread queues each of its faces on each of its two pictures
REPS = {"hevc": 3, "vp9": 3, "vp8": 7}
THREADS, PICTURES, POOL_SLOTS = 4, 2, 64


@pytest.mark.parametrize("codec", PF.CODECS)
def test_frame_threads(codec, delay):
    """Every call of a face here issues at least one launch that takes a progress-pool slot (its counters, or the staged picture
    structs), so the calls counted below are a lower bound of the slot-taking launches queued: at least 96, against 64 slots.  The
    VP8 faces and VP9 intra put several ticket-grid launches in flight at once; the others recycle slots that hold staged structs.
    The threads start queueing together (a barrier), each behind a delay on its own stream, so the streams fill before they drain."""
    torch = _torch()
    L = _lib()
    names = PF.of_codec(codec)
    # the model once per distinct picture: two per thread, seeded differently per thread
    built = [[PF.make(n, PF.SEED[n] + 100 * (k + 1) + j) for j in range(PICTURES) for n in names] for k in range(THREADS)]
    torch.cuda.synchronize()
    errs, calls = [], [0] * THREADS
    gate = threading.Barrier(THREADS)

    def worker(k):
        try:
            assert L.ffhip_set_device(0) == 0
            st = C.c_void_p()
            assert L.ffhip_stream_create(C.byref(st)) == 0
            runs = []
            for _ in range(REPS[codec]):
                for f in built[k]:
                    g = f.fresh()
                    g.upload(torch)                 # fresh input and output tensors for every call
                    runs.append(g)
            gate.wait(60)                           # every thread's uploads are queued ...
            if k == 0:
                torch.cuda.synchronize()            # ... and done: the only device-wide wait
            gate.wait(60)
            with torch.cuda.stream(torch.cuda.ExternalStream(st.value)):
                delay.queue()
            for g in runs:                          # queued back to back: no synchronisation until all are in
                g.call(st.value)
                calls[k] += 1
            assert L.ffhip_stream_synchronize(st) == 0, L.ffhip_last_error()
            for g in runs:
                g.compare()
            assert L.ffhip_stream_destroy(st) == 0
        except Exception as e:  # noqa: BLE001
            gate.abort()
            errs.append("thread %d: %r" % (k, e))
    ts = [threading.Thread(target=worker, args=(k,)) for k in range(THREADS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert sum(calls) >= 96 > POOL_SLOTS and sum(calls) == THREADS * PICTURES * len(names) * REPS[codec]


@pytest.mark.parametrize("codec", PF.CODECS)
def test_first_use_on_a_created_stream(codec):
    """first-use table uploads and the creation of the progress pool under a non-blocking stream: a fresh child process (never an
    exec of this one, which holds the GPU), one at a time"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "picture_stream_child.py"), codec], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, "picture_stream_child.py %s exited with %d:\n%s" % (codec, r.returncode, r.stdout)
    assert "%d faces ok" % len(PF.of_codec(codec)) in r.stdout, r.stdout
