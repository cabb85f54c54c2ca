"""The native TensorBoard event files (srgan_amd/summary_events.py) and the summary writer's use of them, on the host: CRC32C
known answers, the exact bytes of two events, an independent decode with google.protobuf, the record framing, the hand-written
PNGs against the byte rule, the NumPy form of the histogram contract against np.histogram, the writer and the command line."""
import glob
import math
import os
import re
import socket
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def events():
    import srgan_amd  # noqa: F401
    from srgan_amd import summary_events
    return summary_events


@pytest.fixture()
def native(monkeypatch):
    """utility.SummaryWriter on the native path, whatever is installed: ``import tensorboardX`` raises ImportError."""
    import srgan_amd  # noqa: F401
    from srgan_amd import utility
    monkeypatch.setitem(sys.modules, 'tensorboardX', None)
    return utility


def only_file(directory):
    files = glob.glob(os.path.join(directory, 'events.out.tfevents.*'))
    assert len(files) == 1, files
    return files[0]


# ---------------------------------------------------------------------------------------------------------------- CRC32C
def test_crc32c_known_answers(events):
    answers = {b'123456789': 0xE3069283, bytes(32): 0x8A9136AA, b'\xff' * 32: 0x62A8AB43, bytes(range(32)): 0x46DD794E,
               bytes(range(31, -1, -1)): 0x113FDB5C}
    for data, crc in answers.items():
        assert events.crc32c(data) == crc, data
    assert events.crc32c(b'') == 0
    assert events.masked_crc32c(b'123456789') == 0xC78AB0E5
    data = bytes(range(256)) * 3
    for cut in (0, 1, 100, len(data)):
        assert events.crc32c(data[cut:], events.crc32c(data[:cut])) == events.crc32c(data)
    assert events.crc32c(bytearray(data)) == events.crc32c(memoryview(data)) == events.crc32c(data)


# ----------------------------------------------------------------------------------------------------------- exact bytes
def test_the_exact_bytes_of_two_events(events):
    """Produced with google.protobuf from the schema in summary_events.FIELDS."""
    scalar = events.encode_event(1.5, 3, values=[events.encode_value('a', simple_value=0.5)])
    assert scalar.hex() == '09000000000000f83f10032a0a0a080a0161150000003f'
    version = events.encode_event(1.5, file_version='brain.Event:2')
    assert version.hex() == '09000000000000f83f1a0d627261696e2e4576656e743a32'
    framed = events.frame_record(version)
    assert framed[:8] == struct.pack('<Q', len(version)) and framed[12:-4] == version and len(framed) == len(version) + 16
    assert struct.unpack('<I', framed[8:12])[0] == events.masked_crc32c(framed[:8])
    assert struct.unpack('<I', framed[-4:])[0] == events.masked_crc32c(version)


def protobuf_classes():
    """The five messages as dynamic descriptors: nothing of this package takes part in the decode."""
    pytest.importorskip('google.protobuf')
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    T = descriptor_pb2.FieldDescriptorProto
    file = descriptor_pb2.FileDescriptorProto(name='srgan_events_test.proto', package='srgan_events_test', syntax='proto3')

    def message(name, fields, oneof=None):
        m = file.message_type.add(name=name)
        if oneof:
            m.oneof_decl.add(name=oneof)
        for field_name, number, kind, label, type_name, in_oneof in fields:
            f = m.field.add(name=field_name, number=number, type=kind, label=label)
            if type_name:
                f.type_name = '.srgan_events_test.' + type_name
            if in_oneof:
                f.oneof_index = 0
    one, many = T.LABEL_OPTIONAL, T.LABEL_REPEATED
    message('HistogramProto', [('min', 1, T.TYPE_DOUBLE, one, None, False), ('max', 2, T.TYPE_DOUBLE, one, None, False),
                               ('num', 3, T.TYPE_DOUBLE, one, None, False), ('sum', 4, T.TYPE_DOUBLE, one, None, False),
                               ('sum_squares', 5, T.TYPE_DOUBLE, one, None, False),
                               ('bucket_limit', 6, T.TYPE_DOUBLE, many, None, False), ('bucket', 7, T.TYPE_DOUBLE, many, None, False)])
    message('Image', [('height', 1, T.TYPE_INT32, one, None, False), ('width', 2, T.TYPE_INT32, one, None, False),
                      ('colorspace', 3, T.TYPE_INT32, one, None, False), ('encoded_image_string', 4, T.TYPE_BYTES, one, None, False)])
    message('Value', [('tag', 1, T.TYPE_STRING, one, None, False), ('simple_value', 2, T.TYPE_FLOAT, one, None, True),
                      ('image', 4, T.TYPE_MESSAGE, one, 'Image', True), ('histo', 5, T.TYPE_MESSAGE, one, 'HistogramProto', True)],
            oneof='value')
    message('Summary', [('value', 1, T.TYPE_MESSAGE, many, 'Value', False)])
    message('Event', [('wall_time', 1, T.TYPE_DOUBLE, one, None, False), ('step', 2, T.TYPE_INT64, one, None, False),
                      ('file_version', 3, T.TYPE_STRING, one, None, True), ('summary', 5, T.TYPE_MESSAGE, one, 'Summary', True)],
            oneof='what')
    pool = descriptor_pool.DescriptorPool()
    pool.Add(file)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName('srgan_events_test.Event'))


def raw_records(path):
    data, at, out = open(path, 'rb').read(), 0, []
    while at < len(data):
        length = struct.unpack('<Q', data[at:at + 8])[0]
        out.append(data[at + 12:at + 12 + length])
        at += 16 + length
    assert at == len(data)
    return out


def test_an_independent_decode_reads_what_was_written(events, tmp_path):
    Event = protobuf_classes()
    reference = Event(wall_time=1.5, step=3)
    reference.summary.value.add(tag='a', simple_value=0.5)
    assert reference.SerializeToString().hex() == '09000000000000f83f10032a0a0a080a0161150000003f'

    writer = events.EventFileWriter(str(tmp_path))
    steps = [0, 1, 127, 128, 2 ** 32 + 5, 2 ** 62, -1, -2 ** 63]
    for index, step in enumerate(steps):
        writer.add_scalar('Loss/%d' % index, 0.1 * index - 0.3, step, wall_time=10.0 + index)
    picture = np.linspace(0, 1, 3 * 5 * 7, dtype=np.float32).reshape(3, 5, 7)
    writer.add_image('Real', picture, 9, wall_time=20.0)
    record = events.histogram_of_array(np.arange(-50, 51, dtype=np.float32), 30)
    writer.add_histogram('Parameters/D', record, 11, wall_time=21.0)
    writer.close()

    records = raw_records(only_file(str(tmp_path)))
    assert len(records) == 1 + len(steps) + 2
    parsed = [Event.FromString(r) for r in records]
    assert parsed[0].file_version == 'brain.Event:2' and parsed[0].WhichOneof('what') == 'file_version'
    for index, step in enumerate(steps):
        event = parsed[1 + index]
        assert (event.step, event.wall_time) == (step, 10.0 + index)
        (value,) = event.summary.value
        assert value.tag == 'Loss/%d' % index and value.WhichOneof('value') == 'simple_value'
        assert np.float32(value.simple_value) == np.float32(0.1 * index - 0.3)
    (image,) = parsed[-2].summary.value
    assert (parsed[-2].step, image.tag) == (9, 'Real')
    assert (image.image.height, image.image.width, image.image.colorspace) == (5, 7, 3)
    assert np.array_equal(decode_png(image.image.encoded_image_string), events.image_bytes(picture))
    (histogram,) = parsed[-1].summary.value
    histo = histogram.histo
    assert (parsed[-1].step, histogram.tag) == (11, 'Parameters/D')
    assert (histo.min, histo.max, histo.num, histo.sum, histo.sum_squares) == (-50.0, 50.0, 101.0, 0.0, float(sum(i * i for i in range(-50, 51))))
    assert list(histo.bucket_limit) == list(record['edges'][1:]) and list(histo.bucket) == list(record['counts'])
    assert len(histo.bucket) == 30 and sum(histo.bucket) == 101

    # and this package's reader agrees with the independent one, record for record
    own = list(events.read_events(only_file(str(tmp_path))))
    assert [r['step'] for r in own] == [0] + steps + [9, 11]
    assert own[0]['file_version'] == 'brain.Event:2' and 'values' not in own[0]
    assert own[-2]['values'][0]['image'][:3] == (5, 7, 3) and own[-2]['values'][0]['image'][3] == image.image.encoded_image_string
    assert np.array_equal(own[-1]['values'][0]['histo']['bucket'], record['counts'])
    assert own[-1]['values'][0]['histo']['num'] == 101.0


def test_unknown_fields_are_skipped_by_wire_type(events):
    known = events.encode_event(2.0, 7, values=[events.encode_value('t', simple_value=1.0)])
    extras = (b'\x78\x05' +                         # field 15 varint
              b'\x81\x01' + bytes(8) +              # field 16 fixed64
              b'\x8a\x01\x03abc' +                  # field 17 length-delimited
              b'\x95\x01' + bytes(4))               # field 18 fixed32
    decoded = events.decode_message('Event', extras + known + extras)
    assert decoded['step'] == 7 and decoded['wall_time'] == 2.0 and decoded['summary']['value'][0]['tag'] == 't'
    with pytest.raises(ValueError, match='wire type 3'):
        events.decode_message('Event', b'\x7b')     # a group start cannot be skipped


# ---------------------------------------------------------------------------------------------------------------- framing
def test_framing_errors_name_the_offset_and_truncation_is_optional(events, tmp_path):
    writer = events.EventFileWriter(str(tmp_path))
    writer.add_scalar('a', 1.0, 1)
    writer.add_scalar('b', 2.0, 2)
    writer.close()
    path = writer.path
    assert path == only_file(str(tmp_path))
    pattern = r'events\.out\.tfevents\.\d{10}\.%s\.%d\.\d+' % (re.escape(socket.gethostname()), os.getpid())
    assert re.fullmatch(pattern, os.path.basename(path))
    data = open(path, 'rb').read()
    records = list(events.read_events(path))
    assert len(records) == 3 and records[0]['file_version'] == 'brain.Event:2' and records[0]['step'] == 0
    first = 16 + struct.unpack('<Q', data[:8])[0]       # offset of the second record
    second = first + 16 + struct.unpack('<Q', data[first:first + 8])[0]
    broken = str(tmp_path / 'broken')
    for position in (first + 0, first + 9, first + 12 + 3, second - 1):     # length, length CRC, data, data CRC
        damaged = bytearray(data)
        damaged[position] ^= 0x10
        open(broken, 'wb').write(damaged)
        with pytest.raises(ValueError, match=r'checksum mismatch in the record at byte offset %d\b' % first):
            list(events.read_events(broken))
        with pytest.raises(ValueError, match='offset %d' % first):
            list(events.read_events(broken, allow_truncated=True))          # damage is not truncation
    for cut in (len(data) - 1, second + 12 + 2, second + 5):
        open(broken, 'wb').write(data[:cut])
        with pytest.raises(ValueError, match=r'byte offset %d is cut off' % second):
            list(events.read_events(broken))
        assert list(events.read_events(broken, allow_truncated=True)) == records[:2]

    # name order compares the numbers as numbers: the tenth writer of a process in one second comes after its ninth
    names = ['events.out.tfevents.1700000000.host.name.7.10', 'events.out.tfevents.1700000000.host.name.7.9',
             'events.out.tfevents.0999999999.host.name.800.3', 'events.out.tfevents.1700000000.host.name.7.100']
    ordered_directory = tmp_path / 'ordered'
    ordered_directory.mkdir()
    for name in names:
        (ordered_directory / name).write_bytes(b'')
    assert [os.path.basename(p) for p in events.event_files(str(ordered_directory))] == [names[2], names[1], names[0], names[3]]

    other = events.EventFileWriter(str(tmp_path))
    third = events.EventFileWriter(str(tmp_path))
    assert len({path, other.path, third.path}) == 3 and all(os.path.exists(p) for p in (other.path, third.path))
    other.close()
    other.close()                                      # idempotent
    third.close()
    with pytest.raises(ValueError, match='closed'):
        other.add_scalar('late', 1.0, 1)


# -------------------------------------------------------------------------------------------------------------------- PNG
def decode_png(data):
    """uint8 [H, W, channels] of an 8-bit, non-interlaced PNG whose rows all use filter 0."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        length, kind = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + length]
        assert struct.unpack('>I', data[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        at += 12 + length
    assert [kind for kind, _ in chunks] == [b'IHDR', b'IDAT', b'IEND'] and chunks[2][1] == b''
    width, height, depth, colour, compression, filtering, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, compression, filtering, interlace) == (8, 0, 0, 0) and colour in (0, 2)
    channels = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(height, 1 + width * channels)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(height, width, channels)


def byte_rule_table():
    """(values, expected bytes): every k / 255, the float32 neighbours of every tie (k + 0.5) / 255, and the values outside."""
    values, expected = [], []
    for k in range(256):
        values.append(np.float32(k / 255))
        expected.append(k)
    for k in range(255):
        tie = (k + 0.5) / 255
        nearest = np.float32(tie)
        for candidate in (np.nextafter(nearest, np.float32(-1)), nearest, np.nextafter(nearest, np.float32(2))):
            exact = float(candidate) * 255 + 0.5             # exact in float64: 24 + 8 significant bits
            values.append(candidate)
            expected.append(int(math.floor(exact)))
            assert expected[-1] in (k, k + 1)
    for value, byte in ((-0.0, 0), (-1e-9, 0), (-3.0, 0), (1.0 + 1e-6, 255), (7.5, 255), (float('nan'), 0), (float('inf'), 255),
                        (float('-inf'), 0), (1e-45, 0), (0.5 / 255 - 1e-9, 0)):
        values.append(np.float32(value))
        expected.append(byte)
    return np.array(values, dtype=np.float32), np.array(expected, dtype=np.uint8)


def test_png_pixels_follow_the_byte_rule(events):
    values, expected = byte_rule_table()
    assert len(values) == 256 + 3 * 255 + 10 == 1031                        # 1031 = 1031 x 1: a ragged single row
    with np.errstate(invalid='ignore'):
        grey = events.image_bytes(values.reshape(1, 1031))
        assert grey.shape == (1, 1031, 1) and np.array_equal(grey.reshape(-1), expected)
        assert np.array_equal(decode_png(events.encode_png(grey)), grey)
        assert np.array_equal(events.image_bytes(values.reshape(1, 1, 1031)), grey)              # [1, H, W] is grey too
        padded = np.concatenate([values, values[:1]]).reshape(3, 8, 43)                          # RGB, planar in
        colour = events.image_bytes(padded)
    assert colour.shape == (8, 43, 3)
    assert np.array_equal(colour.transpose(2, 0, 1).reshape(-1), np.concatenate([expected, expected[:1]]))
    assert np.array_equal(decode_png(events.encode_png(colour)), colour)
    for shape in ((1, 1), (3, 1, 1), (3, 5, 1), (3, 1, 5), (17, 3)):
        picture = np.random.RandomState(len(shape)).rand(*shape).astype(np.float32)
        pixels = events.image_bytes(picture)
        planar = picture if picture.ndim == 3 else picture[None]
        assert np.array_equal(pixels, np.floor(planar.astype(np.float64) * 255 + 0.5).astype(np.uint8).transpose(1, 2, 0))
        assert np.array_equal(decode_png(events.encode_png(pixels)), pixels)
    bytes_in = np.random.RandomState(5).randint(0, 256, size=(6, 9, 3)).astype(np.uint8)
    assert np.array_equal(decode_png(events.encode_png(events.image_bytes(bytes_in))), bytes_in)
    assert np.array_equal(events.image_bytes(bytes_in[:, :, 0])[:, :, 0], bytes_in[:, :, 0])
    for wrong in (np.zeros((2, 4, 4), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4), np.int32), np.zeros(4, np.float32)):
        with pytest.raises(ValueError):
            events.image_bytes(wrong)


def test_png_reads_back_through_pil(events):
    Image = pytest.importorskip('PIL.Image')
    import io
    colour = np.random.RandomState(1).randint(0, 256, size=(7, 5, 3)).astype(np.uint8)
    decoded = Image.open(io.BytesIO(events.encode_png(colour)))
    assert decoded.mode == 'RGB' and np.array_equal(np.asarray(decoded), colour)
    grey = colour[:, :, :1].copy()
    decoded = Image.open(io.BytesIO(events.encode_png(grey)))
    assert decoded.mode == 'L' and np.array_equal(np.asarray(decoded), grey[:, :, 0])


# ------------------------------------------------------------------------------------------------------------- histograms
def contract_edges(low, high, bins):
    if low == high:
        low, high = low - 0.5, high + 0.5
    edges = [low + i * ((high - low) / bins) for i in range(bins)] + [high]
    return np.array(edges, dtype=np.float64)


def check_against_numpy(events, values, bins):
    record = events.histogram_of_array(values, bins)
    finite = np.asarray(values, dtype=np.float64).reshape(-1)
    finite = finite[np.isfinite(finite)]
    assert record['finite_count'] == finite.size and record['edges'].shape == (bins + 1,) and record['counts'].shape == (bins,)
    if not finite.size:
        assert all(record[key] == 0 for key in ('min', 'max', 'sum', 'sum_squares'))
        assert not record['edges'].any() and not record['counts'].any()
        return record
    assert (record['min'], record['max']) == (finite.min(), finite.max())
    edges = contract_edges(float(finite.min()), float(finite.max()), bins)
    assert np.array_equal(record['edges'], edges)
    assert np.array_equal(record['counts'], np.histogram(finite, bins=edges)[0].astype(np.float64))
    assert record['counts'].sum() == finite.size
    assert math.isclose(record['sum'], math.fsum(finite), rel_tol=0, abs_tol=finite.size * 2.0 ** -53 * math.fsum(np.abs(finite)))
    assert math.isclose(record['sum_squares'], math.fsum(finite * finite), rel_tol=1e-12)
    return record


@pytest.mark.parametrize('bins', [1, 2, 30, 1024])
def test_histogram_of_array_is_numpy_histogram_over_the_contract_edges(events, bins):
    random = np.random.RandomState(bins)
    dyadic = random.randint(-512, 513, size=5000).astype(np.float32) / np.float32(8)       # edges exact for bins 1, 2, 1024
    dyadic[:2] = -64.0, 64.0
    record = check_against_numpy(events, dyadic, bins)
    assert record['sum'] == float(dyadic.astype(np.float64).sum()) and (record['min'], record['max']) == (-64.0, 64.0)
    check_against_numpy(events, random.standard_normal(4097).astype(np.float32), bins)
    check_against_numpy(events, random.standard_normal((33, 7)), bins)                       # float64, any shape
    # values on every edge (x == max among them): each lands in the bin that starts there, the last one in bins - 1
    edges = contract_edges(-1.0, 3.0, bins)
    on_edges = check_against_numpy(events, edges, bins)
    expected = np.ones(bins)
    expected[-1] = 2
    assert np.array_equal(on_edges['counts'], expected)
    mixed = np.array([np.nan, 1.0, np.inf, -np.inf, -0.0, 0.0, 1e-42, -1e-42, 2.5], dtype=np.float32)
    record = check_against_numpy(events, mixed, bins)
    assert record['finite_count'] == 6
    equal = check_against_numpy(events, np.full(100, 2.5, dtype=np.float32), bins)
    assert (equal['edges'][0], equal['edges'][-1]) == (2.0, 3.0) and equal['counts'][bins // 2] == 100
    one = check_against_numpy(events, np.array([-7.0], dtype=np.float32), bins)
    assert one['counts'].sum() == 1 and (one['edges'][0], one['edges'][-1]) == (-7.5, -6.5)
    for nothing in (np.zeros(0, np.float32), np.array([np.nan, np.inf, -np.inf], np.float32)):
        check_against_numpy(events, nothing, bins)
    zeros = events.histogram_of_array(np.array([-0.0, -0.0], dtype=np.float32), bins)        # a zero is reported as +0.0
    assert all(math.copysign(1.0, zeros[key]) == 1.0 and zeros[key] == 0 for key in ('min', 'max', 'sum', 'sum_squares'))


def test_histogram_argument_errors(events):
    for bins in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match='bins'):
            events.histogram_of_array(np.zeros(4, np.float32), bins)
    assert events.check_bins('auto') == 30 and events.check_bins('fd') == 30 and events.check_bins(30.0) == 30
    assert events.histogram_of_array(np.arange(5), 4)['counts'].tolist() == [1, 1, 1, 2]     # integers count as float32


# ------------------------------------------------------------------------------------------------------------- the writer
def test_summary_writer_writes_files_with_a_log_dir_and_none_without(native, events, tmp_path):
    directory = str(tmp_path / 'GAN')
    writer = native.SummaryWriter(directory)
    assert writer._backend is None and writer._events is not None
    writer.step = 4
    writer.add_scalar('Loss', 0.25)
    writer.add_scalar('Loss', 0.1, 6)
    picture = np.random.RandomState(0).rand(3, 4, 6).astype(np.float32)
    writer.add_image('Real', picture)
    writer.add_histogram('Weights', np.arange(10, dtype=np.float32), bins='auto')
    writer.add_histogram('Weights', np.arange(20, dtype=np.float32), 9, bins=4)
    assert writer.scalars == {'Loss': [(4, 0.25), (6, 0.1)]}
    assert writer.images['Real'][0] == 4 and np.array_equal(writer.images['Real'][1], picture)
    step, record = writer.histograms['Weights']
    assert step == 9 and record['counts'].tolist() == [5, 5, 5, 5] and record['finite_count'] == 20

    # before flush() the records may sit in the process; after it a concurrent reader sees all of them
    writer.flush()
    path = only_file(directory)
    seen = list(events.read_events(path))
    assert [r['step'] for r in seen] == [0, 4, 6, 4, 4, 9]
    assert seen[1]['values'] == [{'tag': 'Loss', 'simple_value': 0.25}]
    assert np.float32(seen[2]['values'][0]['simple_value']) == np.float32(0.1)
    height, width, channels, png = seen[3]['values'][0]['image']
    assert (height, width, channels) == (4, 6, 3) and np.array_equal(decode_png(png), events.image_bytes(picture))
    assert len(seen[4]['values'][0]['histo']['bucket']) == 30 and seen[4]['values'][0]['histo']['num'] == 10
    histo = seen[5]['values'][0]['histo']
    assert histo['bucket'].tolist() == [5, 5, 5, 5] and np.array_equal(histo['bucket_limit'], record['edges'][1:])
    assert (histo['min'], histo['max'], histo['sum'], histo['sum_squares']) == (0.0, 19.0, 190.0, 2470.0)
    assert events.scalars(directory) == {'Loss': [(4, 0.25), (6, float(np.float32(0.1)))]}
    writer.add_scalar('Late', 1.0, 10)
    writer.close()
    writer.close()
    assert events.scalars(directory)['Late'] == [(10, 1.0)]
    assert writer.scalars['Late'] == [(10, 1.0)]                             # the memory stays readable

    # a continued run opens a second file in the same directory; scalars() merges them in name order
    again = native.SummaryWriter(directory)
    again.add_scalar('Loss', 0.05, 8)
    again.close()
    assert len(events.event_files(directory)) == 2
    assert [step for step, _ in events.scalars(directory)['Loss']] == [4, 6, 8]

    before = set(os.listdir(str(tmp_path)))
    quiet = native.SummaryWriter()
    quiet.add_scalar('Loss', 0.25, 1)
    quiet.add_image('Real', picture, 1)
    quiet.add_histogram('Weights', np.arange(4, dtype=np.float32), 1)
    quiet.flush()
    quiet.close()
    assert quiet._backend is None and quiet._events is None and quiet.log_dir is None
    assert quiet.scalars == {'Loss': [(1, 0.25)]} and np.array_equal(quiet.images['Real'][1], picture)
    assert quiet.histograms['Weights'][1]['finite_count'] == 4
    assert set(os.listdir(str(tmp_path))) == before


def test_the_command_line_prints_the_scalars(events, tmp_path):
    writer = events.EventFileWriter(str(tmp_path))
    writer.add_scalar('b/Loss', 0.5, 2)
    writer.add_scalar('a/Loss', -1.25, 1)
    writer.add_scalar('b/Loss', 0.1, 3)
    writer.add_image('Real', np.zeros((2, 2), np.float32), 3)
    writer.close()
    environment = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, '-m', 'srgan_amd.summary_events', str(tmp_path)], capture_output=True, text=True,
                          cwd=ROOT, env=environment)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ['a/Loss\t1\t-1.25', 'b/Loss\t2\t0.5', 'b/Loss\t3\t0.100000001']
    usage = subprocess.run([sys.executable, '-m', 'srgan_amd.summary_events'], capture_output=True, text=True, cwd=ROOT,
                           env=environment)
    assert usage.returncode == 2 and 'usage' in usage.stderr
