"""The _fmt face of the H.264 whole-picture inter prediction on the GPU (ffhip_h264_inter_pictures_fmt_dev) at 4:2:2 and 4:4:4, byte
for byte against the model of h264_fmt_picture_gen.py and the host face on whole poisoned buffers (stride padding 0 and 8 samples,
guard rows, inputs unchanged), 17 pictures to a call, 14 bits into both clips; at 4:2:0 and monochrome against the existing face;
and against the picture object made for the format."""
import numpy as np
import pytest

import h264_fmt_picture_gen as F
import h264_inter_picture_gen as GI
import test_gpu_h264_inter_picture as TG
import test_h264_inter_picture_fmt_cpu as TC
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu


def run(pics, wants, fmt, pad=0, what="", face=h264.inter_pictures_fmt):
    torch = TG._torch()
    up = [TG.upload(torch, p, w, pad) for p, w in zip(pics, wants)]
    torch.cuda.synchronize()
    face([a for a, _ in up], pics[0].mb_w, pics[0].mb_h, pics[0].bd, fmt)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    TG.compare(up, what=what)
    return up


@pytest.mark.parametrize("fmt", [2, 3])
def test_picture_sets(fmt):
    """every set of the format, tight rows and rows 8 samples wider: device == model on whole buffers; the host face == model on the
    same pictures (the CPU tier has the sets but the 17 pictures, which run here)"""
    for name in F.INTER_NAMES:
        pics, models = F.inter_set(name)
        if pics[0].fmt != fmt:
            continue
        wants = [m[0] for m in models]
        if name not in F.INTER_CPU_NAMES:
            TC.run_host(pics, wants, fmt, 0, name + " host")
        for pad in (0, 8):
            run(pics, wants, fmt, pad, name)


@pytest.mark.parametrize("fmt", [2, 3])
def test_14_bits_reach_both_clips(fmt):
    rng = np.random.default_rng(9870 + fmt)
    pic = F.InterPicture(rng, 3, 2, fmt, 14, nslices=1, free=True, types="B", p_intra=0.0, weights="explicit")
    s = pic.slices[0]
    s["luma_log2_denom"], s["chroma_log2_denom"], s["use_weight_chroma"] = 1, 1, 1
    s["luma_weight"][..., 0] = np.where(np.arange(64).reshape(32, 2) & 1, 127, -128)
    s["chroma_weight"][..., 0] = np.where(np.arange(128).reshape(32, 2, 2) & 2, 127, -128)
    want = F.inter_model(pic)[0]
    for p in range(3):
        assert (want[p] == 0).sum() > 20 and (want[p] == 16383).sum() > 20
    run([pic], [want], fmt, 4, "14 bits")


@pytest.mark.parametrize("name", ["3x2", "5x4_10", "3x2_mono"])
def test_at_420_and_monochrome_the_bytes_of_the_existing_face(name):
    pics, models = GI.picture_set(name)
    wants = [m[0] for m in models]
    cfi = int(pics[0].chroma)
    a = run(pics, wants, cfi, 4, name + " fmt")
    b = run(pics, wants, cfi, 4, name + " existing", face=h264.inter_pictures)
    for (_, x), (_, y) in zip(a, b):
        for s, t in zip(x["bufs"], y["bufs"]):
            assert bool((s == t).all())
    if not pics[0].chroma:
        run(pics, wants, 1, 0, name + " through idc 1 with NULL chroma")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("fmt", [2, 3])
def test_against_the_picture_object(fmt, bd):
    """the model's calls recorded into an h264.Picture made for the format and flushed give the planes the face gives in one launch"""
    torch = TG._torch()
    rng = np.random.default_rng(9880 + bd + fmt)
    pad = 8
    pic = F.InterPicture(rng, 5, 4, fmt, bd, nslices=3, nrefs=3, types="B")
    # every mode, whatever the draw: all slices get full lists, so a macroblock may sit in any of them; slice 0 has no weights, slices
    # 1 and 2 explicit ones, and the macroblocks go round the three
    pic.slices["num_ref"] = 4
    pic.slices["ref"][:, :, :4] = rng.integers(0, pic.nrefs, (3, 2, 4))
    pic.slices["use_weight"] = [0, 1, 1]
    pic.mb["slice"] = np.arange(len(pic.mb)) % 3
    want, _, cover = F.inter_model(pic)
    refs, strides, step = TG._one_base(torch, pic, pad)
    exp = [TG._padded(w, pad, F.POISON) for w in want]
    face = [torch.full((e.nbytes,), F.POISON, dtype=torch.uint8, device="cuda") for e in exp]
    flushed = [t.clone() for t in face]
    ins = [TG._dev(torch, pic.mb), TG._dev(torch, pic.mvf), TG._dev(torch, pic.slices)]
    arg = dict(dst=face, dst_stride=strides, mb=ins[0], mvf=ins[1], slices=ins[2], mvf_stride=pic.w4, nslices=pic.nslices,
               refs=[dict(base=[refs[p].data_ptr() + k * step[p] for p in range(3)], stride=strides) for k in range(pic.nrefs)])
    obj = h264.Picture(pic.mb_w, pic.mb_h, bit_depth=bd, chroma_format=fmt)
    GI.record(obj, F.picture_records(pic, cover["calls"], strides, step))
    torch.cuda.synchronize()
    h264.inter_pictures_fmt([arg], pic.mb_w, pic.mb_h, bd, fmt)
    obj.flush(flushed, strides, refs)
    torch.cuda.synchronize()
    obj.close()
    for p in range(3):
        a, b = (t.cpu().numpy().view(exp[p].dtype).reshape(exp[p].shape) for t in (face[p], flushed[p]))
        assert np.array_equal(a, exp[p]), "plane %d: the face differs from the model in %d samples" % (p, (a != exp[p]).sum())
        assert np.array_equal(b, exp[p]), "plane %d: the picture object differs from the model in %d samples" % (p, (b != exp[p]).sum())
    assert cover["modes"] == {1, 2, 3, 4} and len(cover["calls"]) > 300
