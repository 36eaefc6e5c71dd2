"""Child of tests/test_gpu_me_bilat_streams.py::test_first_use_in_a_fresh_process: me_bilat_stream_child.py WHAT...

The first calls this process makes into the library create a stream and run the bilateral search faces on it, with the staging of
picture_faces.run_staged: the creation of the progress pool then happens under a non-blocking stream.  Prints one line per run and
"<n> faces ok" and exits 0, or prints the mismatch and exits 1."""
import ctypes as C
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(what):
    import torch

    import picture_faces as PF
    import test_gpu_me_bilat_streams as T
    from ffmpeg_amd import _lib
    assert torch.cuda.is_available()
    faces = [T.MeBilatSearch(w).build() for w in what]      # the model's bytes, before the device is touched
    delay = PF.Delay(torch)
    L = _lib.lib()
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    for f in faces:
        view, ins, keep = PF.run_staged(torch, L, st, [f], delay)
        PF.check_staged(torch, [f], view, ins)
        print("%s ok" % f.what, flush=True)
    assert L.ffhip_stream_destroy(st) == 0
    print("%d faces ok" % len(faces))


if __name__ == "__main__":
    try:
        main(sys.argv[1:])
    except BaseException:  # noqa: BLE001
        traceback.print_exc(file=sys.stdout)
        sys.exit(1)
