"""The staged stream tests of tests/test_gpu_picture_streams.py can fail (no device needed).

Such a test queues, on one stream, the copies that put a face's real inputs in place, the face, and a snapshot of its outputs.  It
passes trivially when the model's output equals what the output tensors held before the call, or when the result does not depend on
the staged input.  For every adapter of picture_faces.py, with the seeds the GPU file uses:
  - every output plane or map of the model differs from its pre-call fill (the sentinel, or for in-place faces the source plane),
    and from a buffer of the poison byte, which is what a face that read poisoned records (all malformed: it writes nothing) leaves;
  - the model's output changes in every compared plane or map when the input samples alone are drawn again with a second seed: the
    weaker form of the check, for all fourteen, since most generators' models do not take malformed records;
  - the stronger form where the model does take them (VP8 reconstruction, whose model applies the kernels' own well-formedness
    rule): run on the records, coefficients, references and planes as they sit on the device before staging, every byte poison, it
    finds no record well formed, writes nothing, and so differs from the model run on the real input in every plane.
These are conditions on the seeds, not measurements."""
import numpy as np
import pytest

import picture_faces as PF


@pytest.fixture(scope="module", params=PF.NAMES)
def face(request):
    return PF.make(request.param)


def _poison_like(a):
    return np.frombuffer(bytes([PF.POISON]) * a.nbytes, a.dtype).reshape(a.shape)


def test_the_model_differs_from_the_pre_call_fill(face):
    wants, fills = face.wants(), face.prefill()
    assert len(wants) == len(fills) and len(wants) >= 1
    for k, (w, f) in enumerate(zip(wants, fills)):
        assert w.shape == f.shape, k
        assert w.size and (np.asarray(w) != np.asarray(f)).any(), "%s output %d equals its pre-call fill" % (face.name, k)


def test_the_model_differs_from_poison(face):
    """A sanity check only: a plane of real samples is all poison with no probability worth the name.  The guard that matters is
    test_the_model_differs_from_the_pre_call_fill: a face that read poisoned records writes nothing and leaves that fill."""
    for k, w in enumerate(face.wants()):
        a = np.ascontiguousarray(w)
        # the generators keep samples as int64; the device holds them at the face's sample size
        if a.dtype == np.int64:
            a = a.astype(np.uint8 if face.bd == 8 else np.uint16)
        assert (a != _poison_like(a)).any(), "%s output %d is all poison" % (face.name, k)


def test_the_model_depends_on_the_staged_input(face):
    wants, alts = face.wants(), face.alt_wants(PF.ALT_SEED)
    assert len(wants) == len(alts)
    for k, (w, a) in enumerate(zip(wants, alts)):
        assert w.shape == a.shape, k
        assert (np.asarray(w) != np.asarray(a)).any(), "%s output %d does not depend on the input samples" % (face.name, k)
    # and drawing them again left the adapter's own picture as it was
    again = PF.make(face.name)
    for w, b in zip(wants, again.wants()):
        assert np.array_equal(w, b)


def test_the_vp8_recon_model_on_poison_writes_nothing():
    """what the early variant of the staged run relies on, for the one face whose model takes malformed records"""
    import test_gpu_vp8_recon as T
    face = PF.make("vp8_recon")
    mbs, co, refs, init = face.frame
    poison = (_poison_like(mbs).copy(), _poison_like(co).copy(), [[_poison_like(p).copy() for p in r] for r in refs], [_poison_like(p).copy() for p in init])
    assert not any(T.RM.well_formed(mb, poison[2], len(poison[1])) for mb in poison[0])
    out = T._want(poison, face.mb_w, face.mb_h)
    for k, (o, before, want) in enumerate(zip(out, poison[3], face.wants())):
        assert np.array_equal(o, before), "plane %d: the model wrote on poisoned records" % k
        assert (o != want).any(), "plane %d: the model on poison equals the model on the real input" % k


def test_every_face_is_listed_once():
    assert len(PF.NAMES) == len(set(PF.NAMES)) == 14
    assert sorted(n for c in PF.CODECS + ["h264"] for n in PF.of_codec(c)) == sorted(PF.NAMES)
    assert len(set(PF.SEED.values())) == 14
