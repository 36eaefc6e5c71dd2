"""Child of tests/test_gpu_picture_streams.py::test_first_use_on_a_created_stream: picture_stream_child.py CODEC (hevc, vp9 or vp8).

The first calls this process makes into the library create a stream and run that codec's whole-picture faces on it, once each, with
the staging of picture_faces.run_staged: first-use table uploads and the creation of the progress pool then happen under a
non-blocking stream.  Prints one line per face and "<n> faces ok" and exits 0, or prints the mismatch and exits 1."""
import ctypes as C
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(codec):
    import torch

    import picture_faces as PF
    from ffmpeg_amd import _lib
    assert torch.cuda.is_available()
    names = PF.of_codec(codec)
    assert names, "unknown codec %r" % codec
    faces = [PF.make(n) for n in names]            # the models, before the library is touched
    delay = PF.Delay(torch)
    L = _lib.lib()
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    t0 = time.time()
    for f in faces:
        view, ins, keep = PF.run_staged(torch, L, st, [f], delay)
        PF.check_staged(torch, [f], view, ins)
        print("%s ok" % f.name, flush=True)
    assert L.ffhip_stream_destroy(st) == 0
    print("%d faces ok in %.2f s on the device side" % (len(faces), time.time() - t0))


if __name__ == "__main__":
    try:
        main(sys.argv[1])
    except BaseException:  # noqa: BLE001
        traceback.print_exc(file=sys.stdout)
        sys.exit(1)
