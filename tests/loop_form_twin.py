"""Which launch sequence a FusedRenderAndCompare runs, restated from the predicates the constructor and its helpers
held before ``pipeline._choose_form`` existed: the booleans one by one, in the order the constructor set them and raised
on them, and the order in which ``__call__`` / ``iteration`` consulted them.  Written from that code, not from
``_choose_form``; tests/test_loop_form_cpu.py compares the two over the whole grid of options."""
BWD_SMALL_TILES = 0x400                  # include/sdfr.h SDFR_BWD_SMALL_TILES (the test asserts both)
SDF_GRAD_DETERMINISTIC = 0x100           # include/sdfr.h SDFR_SDF_GRAD_DETERMINISTIC


def shard(n_views, rank, world):
    """parallel.shard_views: the contiguous shard of `rank`, remainder spread left"""
    base, rem = divmod(n_views, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def decide(V_all, rank, world, grouped, latent, R, narrow, shape_opt, sdf_grad_mode, form, fuse_depth_loss,
           merge_launches, fused_render, fc_in_tail, defer_loss, exchange, W=64, H=48):
    """dict(form, records_form, defer_pose, defer_loss, fused_render, fc_in_tail, big_exchange, det), or ValueError"""
    asked = []                                       # (how often the decoder was asked for its Linear stack)

    def narrow_linear_stack():
        asked.append(1)
        return narrow

    det = bool(sdf_grad_mode & SDF_GRAD_DETERMINISTIC)
    if form not in ("auto", "tail", "records"):
        raise ValueError(f"form must be 'auto', 'tail' or 'records', got {form!r}")
    must = grouped or bool(sdf_grad_mode & BWD_SMALL_TILES)
    if form == "tail" and must:
        raise ValueError("a process group (and BWD_SMALL_TILES) needs the records form")
    n_vec = 8 + latent
    records_form = must or form == "records" or (form == "auto" and V_all >= 8 and bool(fuse_depth_loss)
                                                 and n_vec <= 256)
    if records_form and n_vec > 256:
        raise ValueError(f"the records form's tail handles parameter vectors of up to 256 entries, this decoder's "
                         f"latent makes {n_vec}")
    view_begin, view_end = shard(V_all, rank, world)
    if view_end == view_begin:
        raise ValueError(f"{V_all} view(s) cannot be sharded over {world} ranks: every rank needs one")
    if records_form and not fuse_depth_loss:
        raise ValueError("the sharded loop runs the loss-fused kernels (fuse_depth_loss=True)")
    if det and not records_form:
        raise ValueError("SDF_GRAD_DETERMINISTIC in the loop goes with BWD_SMALL_TILES (or a process group)")
    V = view_end - view_begin
    defer_loss_ = (V < 32) if defer_loss is None else bool(defer_loss)
    defer_pose = bool(merge_launches) and V <= 64
    merge_tail = bool(merge_launches) and V <= 64
    max_pts = W * H
    big_exchange = records_form and shape_opt and exchange == "sdf"
    can_fuse = (merge_tail and not records_form and bool(fuse_depth_loss) and R <= 128 and V <= 8 and max_pts > 0
                and sdf_grad_mode in (0, 1) and 8 + latent <= 256)
    if fused_render and not can_fuse:
        raise ValueError("fused_render needs the tail form over at most 8 views of a grid up to 128^3, the loss-fused "
                         "kernels, sdf_grad_mode 0 / 1 and a parameter vector of at most 256 entries")
    auto = can_fuse and (V <= 4 or not shape_opt)
    fused_render_ = auto if fused_render is None else bool(fused_render)
    can_fc = bool(fused_render_ and shape_opt and narrow_linear_stack())
    if fc_in_tail and not can_fc:
        raise ValueError("fc_in_tail needs fused_render, shape optimisation and a decoder with a narrow Linear stack")
    fc_in_tail_ = can_fc if fc_in_tail is None else bool(fc_in_tail)
    # what __call__ and iteration() then did with them
    tail_form = merge_tail and bool(fuse_depth_loss) and defer_pose and max_pts > 0 and 8 + latent <= 256
    if records_form:
        name = "records"                             # __call__ branched on it first
    elif not tail_form:
        name = "separate"
    elif not fused_render_:
        name = "tail"                                # sdfr_loop_tail
    else:
        name = "fc_in_tail" if fc_in_tail_ else "one_launch"      # sdfr_loop_tail_fused with / without the tape
    return dict(form=name, records_form=records_form, defer_pose=defer_pose, defer_loss=defer_loss_,
                fused_render=fused_render_, fc_in_tail=fc_in_tail_, big_exchange=big_exchange, det=det,
                asked=len(asked), V=V)
