"""The contract of dsrg_eval_confusion_batch (include/dsrg_hip.h) restated in NumPy, and the synthetic inputs that
tests/test_eval_confusion.py and tests/test_validate.py share.  Nothing here needs a GPU.

Per output pixel: scale = (in - 1) / (out - 1) in float64 (0 when out == 1), src = scale * dst, i0 = trunc(src), i1 = i0 + (i0 < in - 1),
l1 = src - i0, l0 = 1 - l1, z = float32(l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)) with every product and sum a
float64 operation of its own (NumPy fuses nothing), pred = the FIRST maximum of z over the labels (np.argmax's rule)."""
import numpy as np


def axis_taps(n_in, n_out):
    """-> (i0, i1, l0, l1) of the n_out output coordinates of an axis with n_in source samples"""
    scale = float(n_in - 1) / float(n_out - 1) if n_out > 1 else 0.0            # one correctly rounded float64 division
    src = np.float64(scale) * np.arange(n_out, dtype=np.float64)
    i0 = src.astype(np.int64)                                                     # (int)src: truncation, src >= 0
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float64)
    return i0, i1, 1.0 - l1, l1


def zoom(scores, Hz, Wz):
    """(C, h, w) float32 -> (C, Hz, Wz) float32: the two-tap blend in float64, rounded once"""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    y0, y1, l0h, l1h = axis_taps(s.shape[1], Hz)
    x0, x1, l0w, l1w = axis_taps(s.shape[2], Wz)
    v00, v01 = s[:, y0][:, :, x0], s[:, y0][:, :, x1]
    v10, v11 = s[:, y1][:, :, x0], s[:, y1][:, :, x1]
    top = l0w[None, None, :] * v00 + l1w[None, None, :] * v01
    bot = l0w[None, None, :] * v10 + l1w[None, None, :] * v11
    return (l0h[None, :, None] * top + l1h[None, :, None] * bot).astype(np.float32)


def predict(scores, Hz, Wz):
    """(C, h, w) -> (Hz, Wz) int64: the first maximum over the labels"""
    return np.argmax(zoom(scores, Hz, Wz), axis=0)


def counters(scores, labels, C, ignore_label=255.0, rule_lt=False, B=None):
    """scores (>= B, C, h, w) f32, labels (B, 1, Hz, Wz) or (B, Hz, Wz) f32 -> the C*C + 1 int64 counters"""
    labels = np.asarray(labels, dtype=np.float32)
    labels = labels.reshape(labels.shape[0], labels.shape[-2], labels.shape[-1])
    B = labels.shape[0] if B is None else B
    hist = np.zeros(C * C + 1, dtype=np.int64)
    for b in range(B):
        lab = labels[b]
        pred = predict(scores[b], lab.shape[0], lab.shape[1])
        keep = (lab < np.float32(C)) if rule_lt else (lab != np.float32(ignore_label))
        with np.errstate(invalid="ignore"):
            exact = keep & (lab >= 0) & (lab < np.float32(C)) & (np.floor(lab) == lab)
        hist[C * C] += int(np.count_nonzero(keep & ~exact))
        g = lab[exact].astype(np.int64)
        hist[:C * C] += np.bincount(g * C + pred[exact], minlength=C * C)
    return hist


def make_scores(rng, B, C, h, w, ties):
    """float32 (B, C, h, w).  ties: small integers with every odd plane a copy of the plane before it (where there is one), so that
    exact ties occur at source pixels AND at every blended pixel between them; else Gaussian"""
    if not ties:
        return rng.standard_normal((B, C, h, w)).astype(np.float32)
    s = rng.integers(-2, 3, (B, C, h, w)).astype(np.float32)
    s[:, 1::2] = s[:, 0:2 * (C // 2):2]
    return s


def make_labels(rng, B, C, Hz, Wz):
    """float32 (B, 1, Hz, Wz) of integral values: ids in range, an ignore (255) rectangle per image, a sprinkle of values >= C (C
    itself and 200), and — with more than one image — image 1 ignored as a whole"""
    lab = rng.integers(0, C, (B, 1, Hz, Wz)).astype(np.float32)
    for b in range(B):
        y, x = int(rng.integers(0, Hz)), int(rng.integers(0, Wz))
        lab[b, 0, y:y + max(1, Hz // 3), x:x + max(1, Wz // 2)] = 255.0
    over = rng.random((B, 1, Hz, Wz))
    lab[over < 0.03] = float(C)
    lab[over > 0.98] = 200.0
    if B > 1:
        lab[1] = 255.0
    return lab


def write_val_files(tmp_path, rng, sizes, nclass=21):
    """PNG image / label pairs and a list file -> (list path, root, [label arrays]).  Images: 16 x 16 blocks of random colours under
    a little noise (regions a network can tell apart); labels: ids below nclass with a 255 rectangle"""
    from PIL import Image
    lines, labels = [], []
    for k, (H, W) in enumerate(sizes):
        blocks = rng.integers(0, 256, ((H + 15) // 16, (W + 15) // 16, 3))
        im = np.kron(blocks, np.ones((16, 16, 1), dtype=np.int64))[:H, :W] + rng.integers(-20, 21, (H, W, 3))
        Image.fromarray(np.clip(im, 0, 255).astype(np.uint8)).save(str(tmp_path / ("val_im%d.png" % k)))
        lab = rng.integers(0, nclass, (H, W), dtype=np.uint8)
        lab[H // 4:H // 2, W // 3:W // 3 + 7] = 255
        Image.fromarray(lab, mode="L").save(str(tmp_path / ("val_lab%d.png" % k)))
        labels.append(lab)
        lines.append("/val_im%d.png /val_lab%d.png\n" % (k, k))
    lst = tmp_path / "val.txt"
    lst.write_text("".join(lines))
    return str(lst), str(tmp_path), labels


def padded_labels(labels, crop, ignore_label=255):
    """[(H, W) uint8] -> (n, 1, crop, crop) float32 with ignore_label off the image (what dsrg_train_f_input_batch writes at top = left = 0)"""
    out = np.full((len(labels), 1, crop, crop), float(ignore_label), dtype=np.float32)
    for b, lab in enumerate(labels):
        out[b, 0, :lab.shape[0], :lab.shape[1]] = lab
    return out
