"""The storage forms of a FingerprintLibrary: how its rows are held, indexed, written and scored.

A library holds exactly one form object, and everything that depends on the form is asked of it:
  empty()                         the stored tuple of a library without rows
  chunk(*data)                    appended data, checked -> (its rows, a call that gives its tuple on the device)
  encode(rows)                    the f32 rows of one model call -> their tuple
  index(stored)                   the index over the stored tuple; it shares the library's tensor
  held_tensors(stored)            the device tensors of the form that count towards nbytes
  save(out_dir, stored, meta)     the form's files and its library.json entries
  read(lib_dir, meta)             those files, checked -> (their shape, finish(device, stride) -> (form, chunk()'s data))
  identify / cross_match          the form's op for dense queries at the catalogue's speed
  is_half, is_compact, missing    its name in the refusals, and what to use when a call needs this form
FlatForm (f32 rows, every row_stride-th of a track), HalfForm (bf16 rows) and CompactForm (IVF-PQ codes and their
quantiser).  Every op and index class is looked up in ops (or ivfpq) when it is called."""
import os

import numpy as np
import torch

from . import ivfpq, ops

FORMAT = 1                   # the files of a flat library
FORMAT_COMPACT = 2           # the files of a compact library
FORMAT_THIN = 3              # the files of a flat library that keeps every row_stride-th row ("row_stride" in library.json)
FORMAT_HALF = 5              # the files of a half library (bf16 rows as uint16 bit patterns; 4 is refused, as it always was)


class _RowsForm:
    """What the two forms that store one (n, 128) tensor of rows share."""
    is_half = is_compact = False

    def __init__(self, device, stride=1):
        self.device, self.stride = device, int(stride)

    def empty(self):
        return (torch.zeros((0, 128), dtype=self.dtype, device=self.device),)

    def held_tensors(self, stored):
        return list(stored)


class FlatForm(_RowsForm):
    """f32 rows, searched by an ops.FlatL2Index (772 bytes a row); stride D: row j of a track is its segment j * D."""
    dtype = torch.float32

    def chunk(self, rows):
        rows = torch.as_tensor(rows).to(self.device, torch.float32).reshape(-1, 128)
        return rows.shape[0], lambda: (rows.contiguous(),)

    def encode(self, rows):
        return (rows,)

    def index(self, stored):
        index = ops.FlatL2Index(d=128, device=self.device)
        index.add(stored[0])
        return index

    def save(self, out_dir, stored, meta):
        from .fpdb import _write_memmap
        if self.stride != 1:
            meta["format"], meta["row_stride"] = FORMAT_THIN, self.stride
        _write_memmap(os.path.join(out_dir, "library"), stored[0].cpu().numpy().reshape(-1, 128))

    @classmethod
    def read(cls, lib_dir, meta):
        shape = tuple(int(v) for v in np.load(os.path.join(lib_dir, "library_shape.npy")))

        def finish(device, stride):
            rows = np.fromfile(os.path.join(lib_dir, "library.mm"), dtype=np.float32).reshape(shape) if shape[0] else \
                np.zeros((0, 128), np.float32)
            return cls(device, stride), (torch.from_numpy(rows),)
        return shape, finish

    def identify(self, stored, *tail, **kw):
        if self.stride != 1:
            return ops.identify_thin(stored[0], *tail, self.stride, **kw)
        return ops.identify(stored[0], *tail, **kw)

    def cross_match(self, stored, *tail, **kw):
        return ops.cross_match(stored[0], *tail, **kw)


class HalfForm(_RowsForm):
    """bf16 rows, searched by an ops.HalfL2Index that shares them (260 bytes a row with its norms)."""
    dtype, is_half = torch.bfloat16, True
    missing = "this is no half library (bf16 rows); halve() makes one of a flat library"

    def chunk(self, rows_bf16):
        if isinstance(rows_bf16, np.ndarray) and rows_bf16.dtype == np.uint16:      # bit patterns, as save() writes them
            rows_bf16 = torch.from_numpy(np.ascontiguousarray(rows_bf16).view(np.int16)).view(torch.bfloat16)
        rows = torch.as_tensor(rows_bf16)
        if rows.dtype != torch.bfloat16 or rows.dim() != 2 or rows.shape[1] != 128:
            raise ValueError(f"the rows of a half library must be (n, 128) torch.bfloat16 (or their uint16 bit patterns "
                             f"in a numpy array), not {tuple(rows.shape)} {rows.dtype}")
        return rows.shape[0], lambda: (rows.detach().to(self.device).contiguous(),)

    def encode(self, rows):
        return (ops.rows_to_bf16(rows),)

    def index(self, stored):
        index = ops.HalfL2Index(d=128, device=self.device)
        index.add(stored[0])
        return index

    def save(self, out_dir, stored, meta):
        bits = stored[0].cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
        np.save(os.path.join(out_dir, "library_half.npy"), bits.reshape(-1, 128))
        meta["format"] = FORMAT_HALF

    @classmethod
    def read(cls, lib_dir, meta):
        bits = np.load(os.path.join(lib_dir, "library_half.npy"))
        if bits.dtype != np.uint16 or bits.ndim != 2 or bits.shape[1] != 128:
            raise ValueError(f"{lib_dir}: library_half.npy must be (n, 128) uint16, not {bits.shape} {bits.dtype}")
        return bits.shape, lambda device, stride: (cls(device), (bits,))

    def identify(self, stored, *tail, **kw):
        return ops.identify_half(stored[0], *tail, **kw)

    def cross_match(self, stored, *tail, **kw):
        return ops.cross_match_half(stored[0], *tail, **kw)


class CompactForm:
    """IVF-PQ codes in row order (list_id int32, codes uint8) with their quantiser, searched by an ivfpq.IVFPQIndex over
    the same codes (2 M + 20 bytes a row); nprobe: the lists that index probes."""
    is_half, is_compact = False, True
    missing = "this is a flat library (f32 rows); compress() makes a compact one"

    def __init__(self, device, quantiser, nprobe):
        cent = torch.as_tensor(quantiser["centroids"]).to(device, torch.float32).contiguous()
        books = torch.as_tensor(quantiser["codebooks"]).to(device, torch.float32).contiguous()
        M = int(books.shape[0]) if books.dim() == 3 else 0
        if M not in ops.IDENTIFY_PQ_M or cent.dim() != 2 or cent.shape[1] != 128 or cent.shape[0] < 1 or \
                tuple(books.shape) != (M, 256, 128 // M):
            raise ValueError(f"a compact library needs centroids (nlist, 128) and codebooks (M, 256, 128 // M) with M "
                             f"one of {ops.IDENTIFY_PQ_M}, not {tuple(cent.shape)} and {tuple(books.shape)}")
        self.device, self.centroids, self.codebooks, self.M, self.nprobe = device, cent, books, M, int(nprobe)
        self._encoder = None                       # the index that encodes rows, made on first use

    def quantiser(self):
        return {"centroids": self.centroids, "codebooks": self.codebooks}

    def empty(self):
        return (torch.zeros(0, dtype=torch.int32, device=self.device),
                torch.zeros((0, self.M), dtype=torch.uint8, device=self.device))

    def chunk(self, list_id, codes):
        M, nlist = self.M, int(self.centroids.shape[0])
        codes, list_id = torch.as_tensor(codes), torch.as_tensor(list_id).reshape(-1)
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != M:
            raise ValueError(f"codes must be (n, {M}) uint8, not {tuple(codes.shape)} {codes.dtype}")
        if list_id.shape[0] != codes.shape[0] or list_id.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{list_id.shape[0]} list ids ({list_id.dtype}) for {codes.shape[0]} rows of codes")
        if list_id.numel() and not 0 <= int(list_id.min()) <= int(list_id.max()) < nlist:
            raise ValueError(f"a list id lies outside [0, {nlist})")
        return codes.shape[0], lambda: (list_id.to(self.device, torch.int32).contiguous(),
                                        codes.to(self.device).contiguous())

    def encode(self, rows):
        """f32 rows on the device -> (list_id int32, codes uint8) with the form's quantiser (csrc/ivfpq.hip)."""
        if self._encoder is None:
            self._encoder = ivfpq.IVFPQIndex.from_codes(self.quantiser(), torch.zeros(0, dtype=torch.int32),
                                                        torch.zeros((0, self.M), dtype=torch.uint8), self.device)
        a, codes = self._encoder.encode(rows)
        return a.to(torch.int32), codes

    def index(self, stored):
        return ivfpq.IVFPQIndex.from_codes(self.quantiser(), *stored, self.device, self.nprobe)

    def held_tensors(self, stored):
        return list(stored) + [self.centroids, self.codebooks]

    def save(self, out_dir, stored, meta):
        cent, books = self.centroids.cpu().numpy(), self.codebooks.cpu().numpy()
        np.save(os.path.join(out_dir, "library_codes.npy"), stored[1].cpu().numpy())
        np.save(os.path.join(out_dir, "library_lists.npy"), stored[0].cpu().numpy().astype(np.int32))
        np.savez(os.path.join(out_dir, "library_pq.npz"), centroids=cent, codebooks=books)
        meta["format"] = FORMAT_COMPACT
        meta["index"] = {"type": "ivfpq", "nlist": int(cent.shape[0]), "M": self.M, "nprobe": self.nprobe}

    @classmethod
    def read(cls, lib_dir, meta):
        if meta.get("index", {}).get("type") != "ivfpq":
            raise ValueError(f"{lib_dir}: a format {FORMAT_COMPACT} library with index {meta.get('index')!r}")
        codes = np.load(os.path.join(lib_dir, "library_codes.npy"))
        lists = np.load(os.path.join(lib_dir, "library_lists.npy"))

        def finish(device, stride):
            with np.load(os.path.join(lib_dir, "library_pq.npz")) as pq:
                quantiser = {"centroids": torch.from_numpy(pq["centroids"]), "codebooks": torch.from_numpy(pq["codebooks"])}
            return cls(device, quantiser, meta["index"]["nprobe"]), (torch.from_numpy(lists), torch.from_numpy(codes))
        return codes.shape, finish

    def identify(self, stored, *tail, **kw):
        return ops.identify_pq(*stored, self.centroids, self.codebooks, *tail, **kw)

    def cross_match(self, stored, *tail, **kw):
        return ops.cross_match_pq(*stored, self.centroids, self.codebooks, *tail, **kw)


FORMS = {FORMAT: FlatForm, FORMAT_COMPACT: CompactForm, FORMAT_THIN: FlatForm, FORMAT_HALF: HalfForm}
