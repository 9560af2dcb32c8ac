"""numpy restatement of what grafp_identify_pq_f32 (csrc/identify_pq.hip, include/grafp_hip.h) decodes: the contract of
the whole op is identify_ref(decode(list_id, codes, centroids, codebooks), ...) of tests/_identify_ref.py."""
import numpy as np


def decode(list_id, codes, centroids, codebooks):
    """dec[r][j] = centroids[list_id[r]][j] + codebooks[m][codes[r][m]][c], m = j // dsub, c = j % dsub: one f32 add per
    element.  list_id (n), codes (n, M) uint8, centroids (nlist, 128) f32, codebooks (M, 256, dsub) f32 -> (n, 128) f32."""
    list_id = np.asarray(list_id, np.int64).reshape(-1)
    codes = np.asarray(codes)
    centroids, codebooks = np.asarray(centroids, np.float32), np.asarray(codebooks, np.float32)
    M = codebooks.shape[0]
    assert codes.dtype == np.uint8 and codes.shape == (len(list_id), M) and codebooks.shape[1:] == (256, 128 // M)
    words = codebooks[np.arange(M)[None, :], codes.astype(np.int64)]                 # (n, M, dsub)
    out = centroids[list_id] + words.reshape(len(list_id), 128)
    assert out.dtype == np.float32
    return out
