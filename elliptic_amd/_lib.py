"""ctypes binding of the C ABI declared in include/ellgpu.h, include/ellgpu_ext.h, include/ellgpu_ext2.h,
include/ellgpu_ext3.h, include/ellgpu_ext4.h, include/ellgpu_addn.h and elliptic_amd/include/ellgpu_edsum.h.

`load()` opens the in-tree libellgpu.so (built by __graft_entry__.build() /
elliptic_amd/build.py with hipcc for gfx950).  There is no fallback of any
kind: if the library is missing this raises, and if it loads on a machine
without a usable MI355X, `Context()` raises from ellgpu_ctx_create.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "lib", "libellgpu.so")

c_u8p = ctypes.c_void_p      # raw addresses (numpy .ctypes.data / torch .data_ptr())

_SIGS = {
    "ellgpu_version": (ctypes.c_int, []),
    "ellgpu_source_digest": (ctypes.c_char_p, []),
    "ellgpu_last_error": (ctypes.c_char_p, []),
    "ellgpu_curve_id": (ctypes.c_int, [ctypes.c_char_p]),
    "ellgpu_curve_field_bytes": (ctypes.c_int, [ctypes.c_int]),
    "ellgpu_curve_order_bytes": (ctypes.c_int, [ctypes.c_int]),
    "ellgpu_device_count": (ctypes.c_int, []),
    "ellgpu_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "ellgpu_group_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "ellgpu_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "ellgpu_ctx_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "ellgpu_ctx_defer": (ctypes.c_int, [ctypes.c_void_p]),
    "ellgpu_ctx_collect": (ctypes.c_int, [ctypes.c_void_p]),
    "ellgpu_curve_define_short": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                 ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_curve_define_edwards": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                   ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_curve_define_short_domain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                                        ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                        ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_curve_define_edwards_domain": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p,
                                                          ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                                          ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_curve_define_mont": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_ctx_destroy": (None, [ctypes.c_void_p]),
    "ellgpu_ctx_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "ellgpu_ctx_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]),
    "ellgpu_ctx_comb_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ellgpu_base_define": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_u8p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "ellgpu_base_release": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ellgpu_base_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    # one symbol for host and device memory: a `where` flag and the stream close the list
    "ellgpu_mul_base": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
    "ellgpu_mul_base2": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
    # host form only
    "ellgpu_x25519_derive": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ctx_set_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "ellgpu_ctx_get_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
    "ellgpu_debug_field_op": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p]),
    "ellgpu_probe_valu": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
}

# the batch entry points: each ellgpu_X here is exported a second time as ellgpu_X_dev, for device
# buffers, whose prototype is this one plus the stream (added below)
_BATCH = {
    "ellgpu_mul_fixed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p]),
    "ellgpu_mul_var": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_mul_add2": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_point_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_x25519_ladder": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ecdsa_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ecdsa_sign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ecdsa_sign_det": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ecdsa_recover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_ecdsa_verify_wire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_eddsa_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_eddsa_sign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_decompress": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_decode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_encode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p]),
    "ellgpu_validate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_int, c_u8p]),
    "ellgpu_sig_from_der": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_sig_to_der": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, ctypes.c_size_t, c_u8p]),
    "ellgpu_custom_decompress": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_decode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_custom_encode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p]),
    "ellgpu_custom_validate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_int, c_u8p]),
    "ellgpu_custom_verify_wire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_custom_recover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_sign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_sign_det": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_derive": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_derive_wire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_mont_ladder": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_mont_validate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_custom_mont_derive": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_sign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_sign_det": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_decompress": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_int, c_u8p, c_u8p]),
    "ellgpu_custom_ed_decode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_size_t, c_u8p, c_u8p]),
    "ellgpu_custom_ed_validate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_char_p, c_u8p]),
    "ellgpu_custom_ed_derive": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_derive_wire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p]),
    "ellgpu_custom_ed_encode_points": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p]),
}
for _name, (_res, _args) in _BATCH.items():
    _SIGS[_name] = (_res, _args)
    _SIGS[_name + "_dev"] = (_res, _args + [ctypes.c_void_p])

# every symbol include/ellgpu.h declares (tests check the .so exports them all)
SYMBOLS = sorted(_SIGS)

# the entry points added after that table was recorded: include/ellgpu_ext.h, a table of its own
# (tests/golden/binding_sigs_ext.json)
_EXT_SIGS = {
    "ellgpu_ed_base_define": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_u8p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
}
EXT_SYMBOLS = sorted(_EXT_SIGS)

# ... and after that one: include/ellgpu_ext2.h, a third table (tests/golden/binding_sigs_ext2.json)
_EXT2_SIGS = {
    "ellgpu_ecdsa_verify_base": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
}
EXT2_SYMBOLS = sorted(_EXT2_SIGS)

# ... and include/ellgpu_ext3.h, a fourth table (tests/golden/binding_sigs_ext3.json)
_EXT3_SIGS = {
    "ellgpu_eddsa_verify_base": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, c_u8p, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
}
EXT3_SYMBOLS = sorted(_EXT3_SIGS)

# ... and include/ellgpu_ext4.h, a fifth table (tests/golden/binding_sigs_ext4.json)
_EXT4_SIGS = {
    "ellgpu_ecdsa_recid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, c_u8p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
}
EXT4_SYMBOLS = sorted(_EXT4_SIGS)

# ... and include/ellgpu_addn.h, a sixth table (tests/golden/addn_binding_sigs.json)
_SUM_SIGS = {
    "ellgpu_mul_sum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
}
SUM_SYMBOLS = sorted(_SUM_SIGS)

# ... and elliptic_amd/include/ellgpu_edsum.h, a seventh table (tests/golden/edsum_binding_sigs.json)
_EDSUM_SIGS = {
    "ellgpu_ed_mul_sum": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, c_u8p, c_u8p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_void_p]),
}
EDSUM_SYMBOLS = sorted(_EDSUM_SIGS)

# ELLGPU_VERSION of the include/ellgpu.h this table was written against: load() refuses any other
# library (a prototype changed -- e.g. ellgpu_ecdsa_verify's out_status -- and a stale table would
# pass garbage for the added arguments)
ABI_VERSION = 0x000200


class EllgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ellgpu error %d: %s" % (code, msg))
        self.code = code


def load(path=None, optional=()):
    path = path or os.environ.get("ELLGPU_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise ImportError(
            "libellgpu.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    lib = ctypes.CDLL(path)
    lib.ellgpu_version.restype = ctypes.c_int
    got = lib.ellgpu_version()
    if got != ABI_VERSION:
        raise ImportError("%s reports ABI version 0x%06x, this binding was written for 0x%06x (include/ellgpu.h "
                          "ELLGPU_VERSION): rebuild the library from this tree" % (path, got, ABI_VERSION))
    for name, (res, args) in (list(_SIGS.items()) + list(_EXT_SIGS.items()) + list(_EXT2_SIGS.items())
                              + list(_EXT3_SIGS.items()) + list(_EXT4_SIGS.items()) + list(_SUM_SIGS.items())
                              + list(_EDSUM_SIGS.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if name in optional:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    lib._path = path
    return lib
