"""UserKNN / ItemKNN (csrc/knn.hip): neighbour lists and their ranking."""
import torch

from ._base import SelfrecHipError, _lib, _p, _stream, check, workspace



KNN_MAX_K = 128                               # srh_knn_neighbours / srh_knn_score_topk keep their lists in LDS


def knn_neighbours(a_indptr, a_indices, t_indptr, t_indices, norm, name_rank, k, shrinkage, query_rows=None):
    """The best k neighbours of rows of a binary matrix A (UserKNN.py:32-57 / ItemKNN.py:32-56 train()):
    sim = (n / (n + s)) * (n / (norm_q * norm_v + 1e-8)), n the shared features, ordered (sim desc, name_rank desc).
    a_* : A as a CSR (int32 device tensors), t_* : its transpose with ascending rows, norm (float64): sqrt of each row's
    degree, name_rank (int32): each row's place in sorted(names).  query_rows (int32, optional): the rows to serve (all
    when None).  Returns (ids (q, k) int32 -1 padded, sims (q, k) float64 0 padded, lengths (q,) int32)."""
    k, shrinkage = int(k), int(shrinkage)
    if not 1 <= k <= KNN_MAX_K:
        raise SelfrecHipError(f"knn_neighbours: topK = {k} -- the kernels keep at most {KNN_MAX_K} neighbours per row")
    if shrinkage < 0:
        raise SelfrecHipError(f"knn_neighbours: negative shrinkage {shrinkage}")
    if shrinkage >= 2 ** 31:
        raise SelfrecHipError(f"knn_neighbours: shrinkage {shrinkage} -- the entry point takes a 32-bit value, below 2**31")
    n_rows = int(a_indptr.numel()) - 1
    if n_rows < 1 or int(norm.numel()) != n_rows or int(name_rank.numel()) != n_rows:
        raise SelfrecHipError("knn_neighbours: a_indptr, norm and name_rank must describe the same rows")
    ptrs = (_p(a_indptr, torch.int32, "a_indptr"), _p(a_indices, torch.int32, "a_indices"),
            _p(t_indptr, torch.int32, "t_indptr"), _p(t_indices, torch.int32, "t_indices"),
            _p(norm, torch.float64, "norm"), _p(name_rank, torch.int32, "name_rank"))
    if query_rows is not None:
        _p(query_rows, torch.int32, "query_rows")
        n_query = int(query_rows.numel())
        if n_query < 1 or int(query_rows.min()) < 0 or int(query_rows.max()) >= n_rows:
            raise SelfrecHipError(f"knn_neighbours: query rows must lie in [0, {n_rows})")
    else:
        n_query = n_rows
    dev = a_indptr.device
    ids = torch.empty((n_query, k), dtype=torch.int32, device=dev)
    sims = torch.empty((n_query, k), dtype=torch.float64, device=dev)
    lens = torch.empty(n_query, dtype=torch.int32, device=dev)
    check(_lib.load().srh_knn_neighbours(*ptrs, n_rows, _p(query_rows), n_query, k, shrinkage, _p(ids), _p(sims), _p(lens),
                                         _stream()), "srh_knn_neighbours")
    return ids, sims, lens


def knn_score_ws(ws_rows, n_items, device):
    """Workspace of srh_knn_score_topk: ws_rows float64 score rows."""
    return torch.empty(int(_lib.load().srh_knn_score_ws_bytes(int(ws_rows), int(n_items))), dtype=torch.uint8, device=device)


def knn_score_topk(mode, users, r_indptr, r_indices, n_items, nbr_ids, nbr_sims, nbr_len, n_top, ws_rows=1024, ws=None,
                   mask_train=True):
    """Masked float64 score rows of the given users and their best n_top items (UserKNN.py:59-81 with mode "user",
    ItemKNN.py:58-81 with mode "item", ranked as base/graph_recommender.py:44-58 ranks them; mask_train=False leaves
    the training items as predict() returns them).

    r_indptr / r_indices: users x items, each user's items in training-file order.  nbr_*: the neighbour lists of
    knn_neighbours (over users for "user", over items for "item").  Returns (ids (q, n_top) int32, scores (q, n_top)
    float64, ws): ranked (score desc, id asc); a row whose n_top + 1 best hold two equal neighbours is marked
    ids[row, 0] = -1 - id and is to be redone in the reference's heap order (find_k_largest_host_f64).  When the users
    fit in ws_rows, ws.view(float64)[:q * n_items] holds their finished score rows after the call."""
    if mode not in ("user", "item"):
        raise SelfrecHipError(f"knn_score_topk: mode {mode!r} (user or item)")
    k_nbr, n_top, n_items = int(nbr_ids.shape[1]), int(n_top), int(n_items)
    if not 1 <= k_nbr <= KNN_MAX_K:
        raise SelfrecHipError(f"knn_score_topk: topK = {k_nbr} -- the kernels keep at most {KNN_MAX_K} neighbours per row")
    if not (n_top >= 1 and n_top + 1 <= min(KNN_MAX_K, n_items)):
        raise SelfrecHipError(f"knn_score_topk: N = {n_top} needs N + 1 <= min({KNN_MAX_K}, {n_items} items)")
    n_query = int(users.numel())
    n_users = int(r_indptr.numel()) - 1
    n_rows = n_users if mode == "user" else n_items
    if int(nbr_ids.shape[0]) != n_rows or int(nbr_len.numel()) != n_rows or tuple(nbr_sims.shape) != tuple(nbr_ids.shape):
        raise SelfrecHipError(f"knn_score_topk: {mode} mode wants neighbour lists of {n_rows} rows")
    ptrs = (_p(users, torch.int32, "users"), _p(r_indptr, torch.int32, "r_indptr"), _p(r_indices, torch.int32, "r_indices"),
            _p(nbr_ids, torch.int32, "nbr_ids"), _p(nbr_sims, torch.float64, "nbr_sims"), _p(nbr_len, torch.int32, "nbr_len"))
    if n_query < 1 or int(users.min()) < 0 or int(users.max()) >= n_users:
        raise SelfrecHipError(f"knn_score_topk: user ids must lie in [0, {n_users})")
    ws_rows = max(1, min(int(ws_rows), n_query))
    need = int(_lib.load().srh_knn_score_ws_bytes(ws_rows, n_items))
    ws = workspace(need, users.device, ws, floor=0)      # (no floor: ws_rows is read back from the buffer's size)
    ws_rows = (ws.numel() * ws.element_size()) // (8 * n_items)
    dev = users.device
    ids = torch.empty((n_query, n_top), dtype=torch.int32, device=dev)
    sc = torch.empty((n_query, n_top), dtype=torch.float64, device=dev)
    check(_lib.load().srh_knn_score_topk(0 if mode == "user" else 1, ptrs[0], n_query, ptrs[1], ptrs[2], n_items, ptrs[3],
                                         ptrs[4], ptrs[5], k_nbr, n_top, int(bool(mask_train)), _p(ws), int(ws_rows), _p(ids),
                                         _p(sc), _stream()),
          "srh_knn_score_topk")
    return ids, sc, ws
