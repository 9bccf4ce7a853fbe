"""What the four training-input entries of the library refuse: per entry one small valid call with made-up device pointers (the
one the argument tests of tests/test_train_input.py, test_train_cuemap.py and test_train_f_scale.py use) and a list of overrides
that each put ONE thing wrong in it.  tools/record_train_input_refusals.py recorded code and message of every row from the library
of commit ec489fe, the last one in which each launcher carried its own copy of the checks, into
tests/golden/train_input_refusals.json; tests/test_train_input_refusals.py replays the rows against the library as built.

Every row is refused before any device call, so nothing here needs a GPU or touches one.  Where a limit cannot be reached alone (an
image of 2^31 bytes cannot lie inside a staging buffer of fewer), the row holds both faults and pins which one is reported."""
import ctypes

FAKE = 256                                                              # a "device pointer" that is never dereferenced
MEAN = [104.0, 117.0, 123.0]

# entry -> (exported function, its arguments in order; the stream, always NULL, follows)
ENTRIES = {
    "s": ("dsrg_train_s_input_batch", ("B", "stage", "nbytes", "off", "H", "W", "coff", "nc", "loff", "nl", "mir", "S", "C", "Hm", "Wm",
                                       "mean", "images", "cues", "labels")),
    "c": ("dsrg_train_s_cuemap_input_batch", ("B", "stage", "nbytes", "off", "H", "W", "coff", "mir", "Sh", "Sw", "C", "Hm", "Wm", "mean",
                                              "ignore", "bgr", "images", "cues", "labels")),
    "f": ("dsrg_train_f_input_batch", ("B", "stage", "nbytes", "off", "loff", "H", "W", "top", "left", "mir", "ch", "cw", "mean", "scale",
                                       "ignore", "data", "label")),
    "fs": ("dsrg_train_f_input_scaled_batch", ("B", "stage", "nbytes", "off", "loff", "H", "W", "Hs", "Ws", "top", "left", "mir", "ch",
                                               "cw", "mean", "scale", "ignore", "data", "label")),
}

_IMAGES = dict(B=3, stage=FAKE, nbytes=4096, off=[0, 256, 512], H=[4, 4, 4], W=[5, 5, 5], mir=[0, 1, 0], mean=MEAN)   # 4 x 5 images
_F = dict(_IMAGES, loff=[2048, 2112, 2176], top=[0, 0, 0], left=[1, 1, 1], ch=17, cw=13, scale=1.0, ignore=255.0, data=FAKE, label=FAKE)
BASELINES = {
    "s": dict(_IMAGES, coff=[1024, 1088, 1152], nc=[5, 5, 5], loff=[3072, 3088, 3104], nl=[2, 2, 2], S=5, C=21, Hm=41, Wm=41,
              images=FAKE, cues=FAKE, labels=FAKE),
    "c": dict(_IMAGES, coff=[1024, 1088, 1152], Sh=5, Sw=6, C=81, Hm=5, Wm=7, ignore=255, bgr=1, images=FAKE, cues=FAKE, labels=FAKE),
    "f": _F,
    "fs": dict(_F, Hs=[6, 6, 6], Ws=[3, 3, 3]),
}


def _b32(**more):
    """32 images in a buffer of 2^16 bytes with every piece inside, so that a total over the batch is the only fault"""
    r = range(32)
    return dict(dict(B=32, nbytes=1 << 16, off=[256 * b for b in r], H=[4] * 32, W=[5] * 32, mir=[b % 2 for b in r]), **more)


def _s32(**more):
    r = range(32)
    return _b32(coff=[8192 + 64 * b for b in r], nc=[5] * 32, loff=[12288 + 16 * b for b in r], nl=[2] * 32, **more)


def _f32(**more):
    return _b32(loff=[12288 + 64 * b for b in range(32)], top=[0] * 32, left=[1] * 32, Hs=[6] * 32, Ws=[3] * 32, **more)


def _each(names, value, tag):
    return [("%s_%s" % (n, tag), {n: value}) for n in names]


_SHARED = ([("B_0", dict(B=0)), ("B_33", dict(B=33)), ("stage_bytes_2^31", dict(nbytes=1 << 31))] +
           _each(("stage", "off", "H", "W", "mir", "mean"), None, "null") +
           [("H_0", dict(H=[4, 0, 4])), ("W_0", dict(W=[5, 5, 0])),
            ("image_2^31_values", dict(B=1, H=[32768], W=[32768], off=[0], mir=[0])),             # (and outside the buffer)
            ("image_one_byte_past_the_end", dict(off=[0, 256, 4096 - 59])),                       # 60 bytes from 4037
            ("image_offset_negative", dict(off=[0, -4, 512]))])
_F_ONLY = (_each(("loff", "top", "left", "data", "label"), None, "null") + _each(("data", "label"), 258, "misaligned") +
           [("ch_0", dict(ch=0)), ("cw_0", dict(cw=0)),
            ("top_negative", dict(top=[0, -1, 0])), ("left_negative", dict(left=[0, 0, -1])),
            ("top_plus_crop_2^31", dict(top=[0, (1 << 31) - 17, 0])), ("left_plus_crop_2^31", dict(left=[0, 0, (1 << 31) - 13])),
            ("label_one_byte_past_the_end", dict(loff=[2048, 2112, 4096 - 19])),                  # 20 bytes from 4077
            ("label_offset_negative", dict(loff=[2048, -1, 2176])),
            ("data_2^31_values", _f32(ch=4800, cw=4800))])                                         # 32 * 3 * 4800^2
OVERRIDES = {
    "s": _SHARED + _each(("coff", "nc", "loff", "nl", "images", "cues", "labels"), None, "null") +
    _each(("images", "cues", "labels"), 258, "misaligned") + _each(("S", "C", "Hm", "Wm"), 0, "0") +
    [("cues_past_the_end", dict(coff=[1024, 1088, 4096 - 56])),                                    # 60 bytes of triplets from 4040
     ("cue_offset_negative", dict(coff=[1024, -4, 1152])), ("cue_offset_misaligned", dict(coff=[1024, 1090, 1152])),
     ("labels_past_the_end", dict(loff=[3072, 3088, 4092])),                                       # 8 bytes of ids from 4092
     ("label_offset_negative", dict(loff=[3072, -4, 3104])), ("label_offset_misaligned", dict(loff=[3072, 3089, 3104])),
     ("cue_count_negative", dict(nc=[5, -1, 5])), ("label_count_negative", dict(nl=[2, 2, -1])),
     ("images_2^31_values", _s32(S=4800)),                                                         # 32 * 3 * 4800^2
     ("cues_2^31_values", _s32(C=1 << 12, Hm=128, Wm=128)),
     ("2^24_workgroups", _s32(C=1 << 19, Hm=1, Wm=1))],                                            # 2^24 planes: a grid of 2^32 threads
    "c": _SHARED + _each(("coff", "images", "cues", "labels"), None, "null") + _each(("images", "cues", "labels"), 258, "misaligned") +
    _each(("Sh", "Sw", "C", "Hm", "Wm"), 0, "0") +
    [("C_97", dict(C=97)), ("ignore_label_-1", dict(ignore=-1)), ("ignore_label_256", dict(ignore=256)), ("bgr_2", dict(bgr=2)),
     ("cue_map_one_byte_past_the_end", dict(coff=[1024, 1088, 4096 - 34])),                        # 35 bytes from 4062
     ("cue_map_offset_negative", dict(coff=[1024, -1, 1152])),
     ("images_2^31_values", _b32(coff=[8192 + 64 * b for b in range(32)], Sh=4800, Sw=4800)),
     ("one_image_2^31_pixels", dict(Sh=46341, Sw=46341)),
     ("cues_2^31_values", _b32(nbytes=1 << 30, coff=[(b + 1) << 20 for b in range(32)], C=96, Hm=1024, Wm=1024)),   # 32 * 96 * 2^20
     ("one_cue_map_2^31_pixels", dict(Hm=46341, Wm=46341))],                                       # (and outside the buffer)
    "f": _F_ONLY + _SHARED,
    "fs": _F_ONLY + _SHARED + _each(("Hs", "Ws"), None, "null") +
    [("Hs_0", dict(Hs=[6, 0, 6])), ("Ws_0", dict(Ws=[3, 3, 0])), ("scaled_2^31_pixels", dict(Hs=[6, 46341, 6], Ws=[3, 46341, 3]))],
}


def rows():
    """-> [(entry, case name, the call's arguments by name)], every baseline with every one of its overrides"""
    return [(e, name, dict(BASELINES[e], **over)) for e in ENTRIES for name, over in OVERRIDES[e]]


def call(L, entry, args):
    """one row through the loaded library L (dsrg_amd._lib.lib()) -> (return code, dsrg_last_error() as str)"""
    def c(name):
        v = args[name]
        if isinstance(v, list):
            return ((ctypes.c_float if name == "mean" else ctypes.c_int32) * len(v))(*v)
        return v
    fn, order = ENTRIES[entry]
    rc = getattr(L, fn)(*([c(n) for n in order] + [None]))
    return rc, L.dsrg_last_error().decode()
