"""Minimal TensorBoard event writer (tf.Event / Summary protos in TFRecord framing) so eval/train
scalars ('Precision @ 1', 'Recall @ 5', 'learning_rate', 'total_loss') land where TensorBoard reads, plus the
histogram and image summaries of the reference trainers (tf.summary.histogram / tf.summary.image) and a small
reader of such files (``read_events``)."""
import os
import socket
import struct
import time
import zlib

import numpy as np

from ..data.tfrecord import TFRecordWriter, _ld, _read_varint, _varint, tf_record_iterator


def _event(wall, step=None, summary=None, file_version=None):
    b = _varint((1 << 3) | 1) + struct.pack("<d", wall)
    if step is not None:
        b += _varint(2 << 3) + _varint(int(step))
    if file_version is not None:
        b += _ld(3, file_version.encode())
    if summary is not None:
        b += _ld(5, summary)
    return b


def _scalar_summary(tag, value):
    v = _ld(1, tag.encode()) + _varint((2 << 3) | 5) + struct.pack("<f", float(value))
    return _ld(1, v)


def _double(field, v):
    return _varint((field << 3) | 1) + struct.pack("<d", float(v))


def histogram_buckets(record):
    """(bucket_limit, bucket) of a TensorStats record, as TF's Histogram::EncodeToProto writes them: the buckets in
    order, every run of empty buckets collapsed into ONE entry carrying the run's last limit and a count of 0."""
    from ..ops.summary import limits
    lim, counts = limits(), record["counts"]
    out_l, out_c = [], []
    i, n = 0, len(counts)
    while i < n:
        end, c = lim[i], int(counts[i])
        i += 1
        if c <= 0:
            while i < n and counts[i] <= 0:
                end, c = lim[i], int(counts[i])
                i += 1
        out_l.append(float(end))
        out_c.append(float(c))
    return out_l, out_c


def _histogram_proto(record):
    """HistogramProto: min=1 max=2 num=3 sum=4 sum_squares=5 (double), bucket_limit=6 bucket=7 (packed double)."""
    bl, bc = histogram_buckets(record)
    return (_double(1, record["min"]) + _double(2, record["max"]) + _double(3, record["num"]) +
            _double(4, record["sum"]) + _double(5, record["sum_squares"]) +
            _ld(6, struct.pack("<%dd" % len(bl), *bl)) + _ld(7, struct.pack("<%dd" % len(bc), *bc)))


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(img):
    """uint8 [H, W, C] (C = 1 grey, 2 grey+alpha, 3 RGB, 4 RGBA) -> PNG bytes (zlib from the standard library)."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (1, 2, 3, 4):
        raise ValueError("uint8 HxWxC image with 1-4 channels expected, got %s %s" % (img.dtype, img.shape))
    h, w, c = img.shape
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * c)], axis=1)  # filter type 0 per row
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
            _png_chunk(b"IDAT", zlib.compress(rows.tobytes())) + _png_chunk(b"IEND", b""))


# ---- Summary.Value encoders (for add_summaries) ---------------------------------------------------------------
def scalar_value(tag, value):
    return _scalar_summary(tag, value)


def histogram_value(tag, record):
    """Summary.Value{tag=1, histo=5} of a TensorStats record (ops/summary.py)."""
    return _ld(1, _ld(1, tag.encode()) + _ld(5, _histogram_proto(record)))


def image_value(tag, img):
    """Summary.Value{tag=1, image=4}; Summary.Image{height=1, width=2, colorspace=3, encoded_image_string=4}."""
    img = np.asarray(img)
    h, w, c = img.shape
    im = (_varint(1 << 3) + _varint(h) + _varint(2 << 3) + _varint(w) + _varint(3 << 3) + _varint(c) +
          _ld(4, encode_png(img)))
    return _ld(1, _ld(1, tag.encode()) + _ld(4, im))


class SummaryWriter:
    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        name = "events.out.tfevents.%d.%s" % (int(time.time()), socket.gethostname())
        self.path = os.path.join(logdir, name)
        self.w = TFRecordWriter(self.path)
        self.w.write(_event(time.time(), file_version="brain.Event:2"))

    def add_scalar(self, tag, value, step):
        self.w.write(_event(time.time(), step, _scalar_summary(tag, value)))

    def add_histogram(self, tag, record, step):
        self.w.write(_event(time.time(), step, histogram_value(tag, record)))

    def add_image(self, tag, img, step):
        self.w.write(_event(time.time(), step, image_value(tag, img)))

    def add_summaries(self, values, step):
        """Many values (scalar_value / histogram_value / image_value) in ONE Event, as one sess.run(summary_op)
        writes them."""
        if values:
            self.w.write(_event(time.time(), step, b"".join(values)))

    def close(self):
        self.w.close()


# ---- reader -------------------------------------------------------------------------------------------------
def _fields(b):
    """(field, wire type, value) of one message: varints as int, fixed64 / fixed32 / length-delimited as bytes."""
    i, n = 0, len(b)
    while i < n:
        key, i = _read_varint(b, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(b, i)
        elif wt == 1:
            v, i = b[i:i + 8], i + 8
        elif wt == 5:
            v, i = b[i:i + 4], i + 4
        elif wt == 2:
            ln, i = _read_varint(b, i)
            v, i = b[i:i + ln], i + ln
        else:
            raise ValueError("unsupported wire type %d" % wt)
        yield f, wt, v


def _decode_histo(b):
    h = dict(min=0.0, max=0.0, num=0.0, sum=0.0, sum_squares=0.0, bucket_limit=[], bucket=[])
    names = {1: "min", 2: "max", 3: "num", 4: "sum", 5: "sum_squares", 6: "bucket_limit", 7: "bucket"}
    for f, wt, v in _fields(b):
        if f in (6, 7):
            vals = struct.unpack("<%dd" % (len(v) // 8), v) if wt == 2 else struct.unpack("<d", v)
            h[names[f]].extend(vals)
        elif f in names:
            h[names[f]] = struct.unpack("<d", v)[0]
    return h


def _decode_image(b):
    im = dict(height=0, width=0, colorspace=0, encoded_image_string=b"")
    names = {1: "height", 2: "width", 3: "colorspace", 4: "encoded_image_string"}
    for f, _, v in _fields(b):
        if f in names:
            im[names[f]] = v
    return im


def read_events(path):
    """The events of one event file: dicts with ``wall_time``, ``step``, ``file_version`` (first record) and
    ``values``, a list of dicts with ``tag`` and one of ``simple_value`` (float), ``histo`` (the HistogramProto
    fields) or ``image`` (height, width, colorspace, encoded_image_string)."""
    out = []
    for rec in tf_record_iterator(path):
        ev = dict(wall_time=0.0, step=0, file_version=None, values=[])
        for f, _, v in _fields(rec):
            if f == 1:
                ev["wall_time"] = struct.unpack("<d", v)[0]
            elif f == 2:
                ev["step"] = v
            elif f == 3:
                ev["file_version"] = v.decode()
            elif f == 5:
                for sf, _, sv in _fields(v):
                    if sf != 1:
                        continue
                    val = {}
                    for vf, _, vv in _fields(sv):
                        if vf == 1:
                            val["tag"] = vv.decode()
                        elif vf == 2:
                            val["simple_value"] = struct.unpack("<f", vv)[0]
                        elif vf == 4:
                            val["image"] = _decode_image(vv)
                        elif vf == 5:
                            val["histo"] = _decode_histo(vv)
                    ev["values"].append(val)
        out.append(ev)
    return out
