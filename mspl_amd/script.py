"""The functions uest_seg_multi_os.py defines ITSELF, with the reference's own positional signatures.

install_dropin() can only alias what the script imports; `get_output`, `merge_outputs`, `update_image_list`,
`generate_pseudo_label` and `generate_pseudo_label_multi_model` are defined in the script's own namespace
(uest_seg_multi_os.py:669-956) and called from its main() (:500, :527).  `patch_script(globals())`, placed after those
definitions (or `install_dropin(script=globals())`), rebinds the five names to the HIP-backed versions, so main() runs
unchanged:

    tgt_train_lst, class_weights = generate_pseudo_label(model, device, save_path, round_idx,
        tgt_num, label_2_id, valid_labels, args, logger, class_encoding, writer)                  # :527

The adapters read from `args` exactly what the reference functions read (`classes`, `data_tgt_train_list`, `use_traversable`,
`use_depth`, `pin_memory`, `class_weighting`, `merge_label_policy`, `eval_training`, `dataset`) plus three optional fields the
reference does not have: `label_batch_size` (default 16; the reference's loader is batch size 1, :746 -- BatchNorm is in eval mode,
so the maps do not depend on it), `label_in_flight` (3), `label_batches_per_launch` (2).  The arguments the reference functions
accept and never use (`tgt_num`, `label_2_id`, `valid_labels`, `class_encoding`, `writer`; the ScoreUpdater built at :733 is
reset and dropped) are accepted and ignored.

The epoch loops of train_segmentation.py live in utilities/train_eval_seg.py and are imported by the script, so install_dropin(
train_loops=True) can alias them: `train_seg_ue` (:164-247, the two-head espdnetue) and `train_seg` (:16-91, the single-head
`--model espnetv2` / `espdnet`) below, both on supervised.GraphedSupervisedStep with the meters on the device; their evaluation
halves `val_seg_ue` / `val_seg` are in mspl_amd.evaluation.
"""
import torch

from . import uest
from .io import update_image_list


def _target_loader(args):
    """uest_seg_multi_os.py:739-746 / :842-849: the target-domain list as a loader of `(image, label[, depth], name, _)` tuples.
    The dataset class is the reference's own (data_loader.segmentation.greenhouse, reached through the drop-in overlay)."""
    if getattr(args, 'dataset', 'greenhouse') != 'greenhouse':
        raise RuntimeError('mspl_amd: the label functions build a loader for --dataset greenhouse only (the reference leaves `ds` '
                           'undefined for anything else, uest_seg_multi_os.py:739-746)')
    from data_loader.segmentation.greenhouse import GreenhouseRGBDSegmentation
    ds = GreenhouseRGBDSegmentation(list_name=args.data_tgt_train_list, train=False,
                                    use_traversable=getattr(args, 'use_traversable', False),
                                    use_depth=getattr(args, 'use_depth', False))
    return torch.utils.data.DataLoader(ds, batch_size=int(getattr(args, 'label_batch_size', 16)), shuffle=False,
                                       pin_memory=bool(getattr(args, 'pin_memory', False)))


def _mode(args):
    """:749-752 / :871-876: `--eval-training` labels with the models in train() mode (BatchNorm with the statistics of each single
    image -- the reference's loader has batch size 1); otherwise eval()."""
    return bool(getattr(args, 'eval_training', False))


def _log(logger, round_idx):
    if logger is not None:
        logger.info('###### Start evaluating target domain train set in round {}! ######'.format(round_idx))      # :777


def generate_pseudo_label(model, device, save_path, round_idx, tgt_num=None, label_2_id=None, valid_labels=None, args=None,
                          logger=None, class_encoding=None, writer=None, testloader=None):
    """uest_seg_multi_os.py:730-830 with its own signature; returns (tgt_train_lst, class_weights float32 on `device`)."""
    eval_training = _mode(args)
    loader = testloader if testloader is not None else _target_loader(args)
    _log(logger, round_idx)
    lst, w = uest.generate_pseudo_label(
        model, loader, save_path, eval_training=eval_training, classes=args.classes, class_weighting=getattr(args, 'class_weighting', 'normal'),
        use_depth=getattr(args, 'use_depth', False), device=device, in_flight=int(getattr(args, 'label_in_flight', 3)),
        batches_per_launch=int(getattr(args, 'label_batches_per_launch', 2)))
    print('class_weights : {}'.format(w.cpu().numpy()))   # :826
    return lst, w.to(device)


def generate_pseudo_label_multi_model(model_list, os_data_list, device, save_path, round_idx, tgt_num=None, label_2_id=None,
                                      valid_labels=None, args=None, logger=None, class_encoding=None, writer=None, testloader=None):
    """uest_seg_multi_os.py:832-956 with its own signature."""
    eval_training = _mode(args)
    loader = testloader if testloader is not None else _target_loader(args)
    _log(logger, round_idx)
    lst, w = uest.generate_pseudo_label_multi_model(
        model_list, os_data_list, loader, save_path, eval_training=eval_training, classes=args.classes,
        merge_label_policy=getattr(args, 'merge_label_policy', 'all'), class_weighting=getattr(args, 'class_weighting', 'normal'),
        use_depth=getattr(args, 'use_depth', False), device=device, in_flight=int(getattr(args, 'label_in_flight', 3)),
        batches_per_launch=int(getattr(args, 'label_batches_per_launch', 1)))
    print('class_weights : {}'.format(w.cpu().numpy()))   # :948
    return lst, w.to(device)


# ---------------------------------------------------------------------------------------------------------------- train() (:958-1089)
_FORCE_RESTATED = False         # tests: send a call that qualifies for the graphed step through the restated body instead


def _fast_path(model, criterion, optimizer, args, add_loss):
    """The settings of the shipped espdnet_greenhouse_uest_multi_os.sh: everything the graphed step (frozen BatchNorm, the uest
    loss at head resolution, Adam on flat buffers) computes.  RGB-D batches (`--use-depth true`) qualify as well: the step takes the
    depth batch as a third static tensor.  RGB-D together with an additional loss (--use-nid) keeps the restated body."""
    from . import losses
    if _FORCE_RESTATED or getattr(args, 'model', None) != 'espdnetue':
        return False
    if not getattr(args, 'use_uncertainty', False) or model.training:
        return False
    if getattr(args, 'use_depth', False) and add_loss is not None:
        return False
    # the additional loss of --use-nid: the drop-in NIDLoss itself (not a subclass, not another callable) with one label bin per
    # class of the model; anything else runs the reference body
    if add_loss is not None and (type(add_loss) is not losses.NIDLoss or add_loss.C != getattr(model, 'classes', None)):
        return False
    if type(criterion) is not losses.UncertaintyWeightedSegmentationLoss:
        return False
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return False
    g = optimizer.param_groups[0]
    return not g.get('amsgrad', False) and not g.get('maximize', False)


def _nid_key(add_loss):
    """What a captured step froze of its additional loss: None without one, else the NIDLoss settings."""
    return None if add_loss is None else (add_loss.K, add_loss.C, float(add_loss.bw_camera), float(add_loss.bw_label))


def _train_fast(trainloader, model, criterion, device, optimizer, tot_iter, args, meters, add_loss=None):
    """The step loop on training.GraphedTrainStep: no .item(), no .cpu(), no synchronize inside.  The caller's optimizer never
    steps (its state stays empty); its hyper-parameters are read into the FlatAdam of the graphed step and its learning rate is
    kept current.  One graphed step per model is kept on the model object and reused across epochs and rounds.  It is keyed on its
    meters and on the additional loss it was captured with: a model whose step was captured without the NID term (or with other
    NIDLoss settings) and that is then trained with it raises -- the captured graph cannot change what it computes.  The same holds
    for the depth batch of `args.use_depth` (batch[2]): a step captured with one must be called with one.  Returns the last batch's
    (images, labels, depths) for the visualisation hook."""
    import weakref
    from . import training
    g = optimizer.param_groups[0]
    state = model.__dict__.setdefault('_mspl_train_loop', {})
    use_depth = bool(getattr(args, 'use_depth', False))
    images = labels = depths = None
    for i_iter, batch in enumerate(trainloader):
        images = batch[0].to(device)
        labels = batch[1].to(device)
        if use_depth:
            depths = batch[2].to(device)
        lr = training.adjust_learning_rate(optimizer, i_iter, tot_iter, args.learning_rate, args.power)        # :982
        gs = state.get('step')
        if gs is None:
            # the first batch shapes the capture and is NOT applied by it (consume_first_batch=False)
            gs = training.GraphedTrainStep(model, images, labels, criterion.class_weights, None, lr=lr, weight_decay=g['weight_decay'],
                                           lanes=int(getattr(args, 'train_lanes', 2)), meters=meters, consume_first_batch=False,
                                           add_loss=add_loss, depth=depths)
            state['step'] = gs
            state['optimizer'] = None
        if gs.meters is not meters:
            raise RuntimeError('mspl_amd.script.train: the graphed step of this model was captured with other meters')
        if _nid_key(gs.add_loss) != _nid_key(add_loss):
            raise RuntimeError('mspl_amd.script.train: the graphed step of this model was captured %s and is now called %s; a captured '
                               'step cannot change its loss (train a fresh model object, or keep add_loss the same across epochs)'
                               % tuple('without an additional loss' if k is None else 'with NIDLoss(image_bin=%d, label_bin=%d, bw_camera=%g, '
                                       'bw_label=%g)' % k for k in (_nid_key(gs.add_loss), _nid_key(add_loss))))
        if state.get('optimizer') is None or state['optimizer']() is not optimizer:
            # a new optimizer object (one per round, :594-598) starts as a fresh torch.optim.Adam would
            gs.reset_optimizer(lr, g['betas'], g['eps'], g['weight_decay'])
            state['optimizer'] = weakref.ref(optimizer)
        if i_iter == 0:
            gs.set_class_weights(criterion.class_weights)        # (new weights after a relabelling round, :527-530)
        gs.optimizer.lr = lr
        if (gs.depth is None) != (depths is None):
            raise RuntimeError('mspl_amd.script.train: the graphed step of this model was captured %s a depth batch and is now called '
                               '%s one; a captured step cannot change its inputs (train a fresh model object)'
                               % (('without', 'with') if gs.depth is None else ('with', 'without')))
        if tuple(images.shape) == tuple(gs.images.shape):
            gs(images, labels, depths)
        else:                                                    # the loader has no drop_last: same FlatAdam, same meters, eager
            training.train_step(model, images, labels, gs.cw, gs.optimizer, None, ce_scale=gs.ce_scale, meters=meters, add_loss=add_loss,
                                depth=depths)
    return images, labels, depths


def _train_restated(trainloader, model, criterion, device, optimizer, tot_iter, args, add_loss, meters):
    """The reference body (:975-1041) on the drop-in modules with the caller's own optimizer; the meters stay on the device."""
    from . import layers, losses, training
    if getattr(args, 'model', None) == 'deeplabv3':
        raise RuntimeError("mspl_amd.script.train: --model deeplabv3 has no backbone in this project (espdnetue / espdnet only)")
    kld_layer = losses.PixelwiseKLD()
    images = labels = depths = None
    for i_iter, batch in enumerate(trainloader):
        images = batch[0].to(device)
        labels = batch[1].to(device)
        if args.use_depth:
            depths = batch[2].to(device)
        optimizer.zero_grad()
        training.adjust_learning_rate(optimizer, i_iter, tot_iter, args.learning_rate, args.power)
        out = model(images, depths) if args.use_depth else model(images)
        if args.model != 'espdnetue':
            raise RuntimeError("mspl_amd.script.train: --model %s returns one head; the loop needs the auxiliary head of 'espdnetue' "
                               "(the reference stops at uest_seg_multi_os.py:1020 with pred_aux unbound)" % (args.model,))
        pred, pred_aux = out
        if args.use_uncertainty:
            kld = kld_layer(pred, pred_aux)
            loss = criterion(pred + 0.5 * pred_aux, labels, kld) * 20 + kld.mean()
        else:
            loss = criterion(pred + 0.5 * pred_aux, labels)
        loss2 = None
        if add_loss is not None:
            loss2 = add_loss(images, pred.to(device))
            loss = loss + loss2
        meters.add(pred, labels, loss, images.size(0), extra=loss2)
        meters.count(images.size(0))
        loss.backward()
        optimizer.step()
        layers.bump_param_epoch()       # (torch.optim bumps the version counters the caches watch; this covers an optimizer that does not)
    return images, labels, depths


def _train(namespace, trainloader, model, criterion, device, interp, optimizer, tot_iter, round_idx, epoch_idx, args, logger, metric,
           class_encoding, writer_idx, class_weights, writer, add_loss):
    from . import training
    state = model.__dict__.setdefault('_mspl_train_loop', {})
    meters = state.get('meters')
    if meters is None:
        meters = state['meters'] = training.TrainMeters(4, device)          # MIOU(num_classes=4), :971
    meters.reset()
    if _fast_path(model, criterion, optimizer, args, add_loss):
        images, labels, depths = _train_fast(trainloader, model, criterion, device, optimizer, tot_iter, args, meters, add_loss)
    else:
        images, labels, depths = _train_restated(trainloader, model, criterion, device, optimizer, tot_iter, args, add_loss, meters)
    r = meters.read()                   # the epoch's one device-to-host copy
    iou = r['inter'] / (r['union'] + 1e-10)                                   # :1050
    miou = iou.mean() * 100 if args.use_traversable else iou[[1, 2, 3]].mean() * 100
    nid_avg = r['extra_sum'] / r['steps'] if (add_loss is not None and r['steps']) else 0.0
    writer.add_scalar('uest/train/loss', r['loss_avg'], writer_idx)
    writer.add_scalar('uest/train/nid_loss', nid_avg, writer_idx)
    writer.add_scalar('uest/train/mean_IoU', miou, writer_idx)
    writer.add_scalar('uest/train/traversable_plant_IoU', iou[0], writer_idx)
    writer.add_scalar('uest/train/other_plant_mean_IoU', iou[1], writer_idx)
    writer.add_scalar('uest/train/artificial_object_mean_IoU', iou[2], writer_idx)
    writer.add_scalar('uest/train/ground_mean_IoU', iou[3], writer_idx)
    writer.add_scalar('uest/train/learning_rate', optimizer.param_groups[0]['lr'], writer_idx)
    ns = namespace if namespace is not None else {}
    visualise = ns.get('in_training_visualization_img')
    if visualise is not None:                                                 # :1072-1078
        if args.use_depth:
            visualise(model, images=images, depths=depths, labels=labels.long(), class_encoding=class_encoding, writer=writer,
                      epoch=writer_idx, data='uest/train', device=device)
        else:
            visualise(model, images=images, labels=labels.long(), class_encoding=class_encoding, writer=writer, epoch=writer_idx,
                      data='uest/train', device=device)
    writer_idx += 1
    print('taking snapshot ...')
    return writer_idx


def train(trainloader, model, criterion, device, interp, optimizer, tot_iter, round_idx, epoch_idx, args, logger, metric,
          class_encoding, writer_idx, class_weights=None, writer=None, add_loss=None):
    """uest_seg_multi_os.py:958-1089 with its own signature; returns writer_idx + 1.  `interp` is ignored (:986), `round_idx`,
    `epoch_idx`, `logger`, `metric` and `class_weights` are accepted and unused, as there.  With the shipped settings (espdnetue, with
    or without `args.use_depth` -- batch[2] is then the depth batch --, --use-uncertainty, a model in eval() mode, the drop-in
    UncertaintyWeightedSegmentationLoss, one-group torch.optim.Adam)
    the steps run on training.GraphedTrainStep with `args.train_lanes` (default 2) micro-batch lanes and the meters are taken
    inside the loss kernel; the caller's Adam then never steps and holds no state.  `add_loss` (--use-nid) may be None or the drop-in
    NIDLoss with label_bin equal to the model's class count: its term is then taken from the low-resolution main head inside the
    same graph (NIDLoss.at_heads), on ONE lane whatever `args.train_lanes` says (the NID histogram couples the images of a batch).
    Everything else -- RGB-D batches together with an additional loss among it -- runs the reference body on the drop-in modules."""
    return _train(None, trainloader, model, criterion, device, interp, optimizer, tot_iter, round_idx, epoch_idx, args, logger, metric,
                  class_encoding, writer_idx, class_weights, writer, add_loss)


def _bound_train(ns):
    """`train` that remembers the script's namespace (its `in_training_visualization_img` is looked up there at call time)."""
    def train(trainloader, model, criterion, device, interp, optimizer, tot_iter, round_idx, epoch_idx, args, logger, metric,
              class_encoding, writer_idx, class_weights=None, writer=None, add_loss=None):
        return _train(ns, trainloader, model, criterion, device, interp, optimizer, tot_iter, round_idx, epoch_idx, args, logger,
                      metric, class_encoding, writer_idx, class_weights, writer, add_loss)
    train.__doc__ = globals()['train'].__doc__
    return train


SCRIPT_FUNCTIONS = {
    'get_output': uest.get_output,                                          # :669
    'merge_outputs': uest.merge_outputs,                                    # :695
    'update_image_list': update_image_list,                                 # :720
    'generate_pseudo_label': generate_pseudo_label,                         # :730
    'generate_pseudo_label_multi_model': generate_pseudo_label_multi_model,  # :832
}


def patch_script(namespace, train=False):
    """Rebind the script-level functions in `namespace` (the script's globals() or its module object).  Returns the names bound.
    train=True also binds `train` (:958), the self-training loop on the graphed step."""
    ns = namespace if isinstance(namespace, dict) else vars(namespace)
    ns.update(SCRIPT_FUNCTIONS)
    if train:
        ns['train'] = _bound_train(ns)
        return sorted(list(SCRIPT_FUNCTIONS) + ['train'])
    return sorted(SCRIPT_FUNCTIONS)


# ------------------------------------------------------------- train_seg_ue() (utilities/train_eval_seg.py:164-247, train_segmentation.py:368)
def _graphed_sgd_path(model_ok, criterion, optimizer, add_criterion, device, use_depth):
    """The settings of the shipped train_segmentation.py runs that supervised.GraphedSupervisedStep computes, for a model that passed
    the caller's test (`model_ok`): the drop-in SegmentationLoss('ce'), no additional criterion, plain momentum SGD over the script's
    2 or 3 learning-rate groups, a CUDA device.  RGB-D batches (use_depth) take the restated body."""
    from . import losses
    if _FORCE_RESTATED or add_criterion is not None or use_depth or not model_ok:
        return False
    if type(criterion) is not losses.SegmentationLoss or criterion.loss_type != 'ce':
        return False
    if type(optimizer) is not torch.optim.SGD or len(optimizer.param_groups) not in (2, 3):
        return False
    for g in optimizer.param_groups:
        if g.get('dampening', 0) != 0 or g.get('nesterov', False) or g.get('maximize', False):
            return False
    try:
        return torch.device(device).type == 'cuda'
    except (RuntimeError, TypeError):
        return False


def _supervised_fast_path(model, criterion, optimizer, add_criterion, device, use_depth=False):
    """_graphed_sgd_path for train_seg_ue: the drop-in two-head ESPDNet-UE with its auxiliary head."""
    from . import models
    two_heads = type(model) is models.ESPDNetwithUncertaintyEstimation and getattr(model, 'aux_layer', -1) >= 0
    return _graphed_sgd_path(two_heads, criterion, optimizer, add_criterion, device, use_depth)


def _train_seg_ue_fast(model, dataset_loader, optimizer, criterion, device, meters, state, heads=2):
    """The step loop on supervised.GraphedSupervisedStep (heads=1: its single-head form, for train_seg): no .item(), no .cpu(), no
    synchronize inside.  The caller's SGD never steps
    (its state stays empty); its groups' hyper-parameters are read into the FlatSGD of the graphed step at every iteration (the
    script writes the learning rates per epoch, train_segmentation.py:353-362).  One graphed step per model is kept on the model
    object and reused across epochs; a new optimizer object starts with zero momentum, as a fresh torch.optim.SGD would."""
    import weakref
    from . import supervised
    if state.get('step') is not None:
        # (an epoch on the restated body in between leaves the caller's own gradient tensors on the parameters)
        state['step'].optimizer.reattach()
    for batch in dataset_loader:
        inputs = batch[0].to(device=device)
        target = batch[1].to(device=device)
        gs = state.get('step')
        if gs is None:
            # the first batch shapes the capture and is NOT applied by it (consume_first_batch=False)
            kw = {} if heads == 2 else {'heads': heads}
            gs = supervised.GraphedSupervisedStep(model, inputs, target, criterion, meters=meters, consume_first_batch=False,
                                                  param_groups=optimizer.param_groups, **kw)
            state['step'] = gs
            state['optimizer'] = None
        if gs.meters is not meters:
            raise RuntimeError('mspl_amd.script.train_seg_ue: the graphed step of this model was captured with other meters')
        gs.set_criterion(criterion)
        if state.get('optimizer') is None or state['optimizer']() is not optimizer:
            if not gs.optimizer.same_partition(optimizer.param_groups):
                raise RuntimeError('mspl_amd.script.train_seg_ue: this optimizer splits the parameters into other groups than the one the '
                                   "graphed step of this model was built from; call script.release_supervised_loop(model) first")
            gs.optimizer.reset(optimizer.param_groups)
            state['optimizer'] = weakref.ref(optimizer)
        for g, src in zip(gs.optimizer.param_groups, optimizer.param_groups):
            g['lr'], g['momentum'], g['weight_decay'] = src['lr'], src['momentum'], src['weight_decay']
        if tuple(inputs.shape) == tuple(gs.inputs.shape):
            gs(inputs, target)
        elif heads == 2:                                         # the loader has no drop_last: same FlatSGD, same meters, eager
            supervised.train_seg_ue_step(model, inputs, target, criterion, gs.optimizer, b=gs.b, meters=meters)
        else:
            supervised.train_seg_step(model, inputs, target, criterion, gs.optimizer, meters=meters, ce_at_head=gs.ce_at_head)


def _train_seg_ue_restated(model, dataset_loader, optimizer, criterion, device, use_depth, add_criterion, weight, meters):
    """The reference body (:179-228) on the drop-in modules with the caller's own optimizer; the meters stay on the device.  (The
    reference also evaluates PixelwiseKLD at :196 and never uses the result; that launch is left out.)"""
    from collections import OrderedDict
    from . import layers, supervised
    for batch in dataset_loader:
        inputs = batch[0].to(device=device)
        target = batch[1].to(device=device)
        outputs = model(inputs, batch[2].to(device=device)) if use_depth else model(inputs)
        if isinstance(outputs, OrderedDict):
            out_aux, outputs = outputs['aux'], outputs['out']
        else:
            out_aux, outputs = outputs[1], outputs[0]
        outputs = outputs + 0.5 * out_aux
        loss = criterion(outputs, target).mean()
        loss2 = None
        if add_criterion is not None:
            loss2 = add_criterion(inputs, outputs.to(device)) * weight
            loss = loss + loss2
        loss = supervised.flood(loss)
        meters.add(outputs, target, loss, inputs.size(0), extra=loss2)
        meters.count(inputs.size(0))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        layers.bump_param_epoch()       # (torch.optim bumps the version counters the caches watch; this covers an optimizer that does not)


def release_supervised_loop(model):
    """Drop what train_seg_ue keeps on the model object between epochs (`model.__dict__['_mspl_supervised_loop']`: the graphed step
    with its static batch, graph and FlatSGD, and the meters, bound to the first call's device and num_classes).  The parameters
    stay where they are (views of the flat buffer, which lives as long as they do)."""
    model.__dict__.pop('_mspl_supervised_loop', None)


def train_seg_ue(model, dataset_loader, optimizer, criterion, num_classes, epoch, device='cuda', use_depth=False, add_criterion=None,
                 weight=1.0, greenhouse_use_trav=False):
    """utilities/train_eval_seg.py:164-247 with its own signature; returns (iou float32[num_classes - 1], average flooded loss), where
    iou = inter / (union + 1e-10) over the epoch's summed areas of the `out + 0.5 * aux` logits (`greenhouse_use_trav` only selects
    a mean the reference computes and drops, :241-245).  With the shipped settings (`_supervised_fast_path`) the iterations run on
    supervised.GraphedSupervisedStep with loss and meters taken in one read of the logits; the caller's SGD then never steps and holds
    no state.  Everything else -- an additional criterion with `weight`, RGB-D batches, other models, losses or optimizers -- runs the
    reference body on the drop-in modules with the caller's optimizer.  Nothing inside the loop synchronises, so the reference's
    running log line of every tenth iteration is not printed; one line follows the epoch.  Meters are per rank.  The graphed step
    and the meters are kept on the model object until release_supervised_loop(model); an epoch on the restated body may come in between
    (the flat gradient views are re-attached at the next graphed epoch), an optimizer with another split of the parameters raises."""
    from . import supervised
    model.train()
    state = model.__dict__.setdefault('_mspl_supervised_loop', {})
    meters = state.get('meters')
    if meters is None:
        meters = state['meters'] = supervised.SupervisedMeters(num_classes - 1, device)       # MIOU(num_classes - 1), :175
    elif meters.classes != num_classes - 1 or meters.areas.device.type != torch.device(device).type:
        raise RuntimeError('mspl_amd.script.train_seg_ue: this model was run with num_classes=%d on %s before; call '
                           'script.release_supervised_loop(model) first' % (meters.classes + 1, meters.areas.device))
    meters.reset()
    print("train_seg_ue()")
    if _supervised_fast_path(model, criterion, optimizer, add_criterion, device, use_depth):
        _train_seg_ue_fast(model, dataset_loader, optimizer, criterion, device, meters, state)
    else:
        _train_seg_ue_restated(model, dataset_loader, optimizer, criterion, device, use_depth, add_criterion, weight, meters)
    r = meters.read()                   # the epoch's one device-to-host copy
    import numpy as np
    iou = (r['inter'] / (r['union'] + 1e-10)).astype(np.float32)            # :240
    nid_avg = r['extra_sum'] / r['steps'] if (add_criterion is not None and r['steps']) else 0.0
    print("Epoch: %d[%d steps]\t\tLoss:%.4f\t\tmiou:%.4f\t\tNID loss:%.4f" % (epoch, r['steps'], r['loss_avg'], iou.mean() * 100, nid_avg))
    return iou, r['loss_avg']


# ------------------------------------------------------------- train_seg() (utilities/train_eval_seg.py:16-91, train_segmentation.py:370-372)
def _single_head_fast_path(model, criterion, optimizer, add_criterion, device, use_depth=False):
    """_graphed_sgd_path for train_seg: the drop-in ESPNetv2Segmentation or ESPDNetSegmentation."""
    from . import models
    one_head = type(model) in (models.ESPNetv2Segmentation, models.ESPDNetSegmentation)
    return _graphed_sgd_path(one_head, criterion, optimizer, add_criterion, device, use_depth)


def _train_seg_restated(model, dataset_loader, optimizer, criterion, device, use_depth, add_criterion, weight, meters):
    """The reference body (:28-69) on the drop-in modules with the caller's own optimizer; the meters stay on the device
    (`nid_losses.update(loss2.item(), 1)` is the meters' `extra`)."""
    from . import layers, supervised
    for batch in dataset_loader:
        inputs = batch[0].to(device=device)
        target = batch[1].to(device=device)
        depth = batch[2].to(device=device) if use_depth else None
        loss, _ = supervised._single_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, meters)
        meters.count(inputs.size(0))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        layers.bump_param_epoch()       # (torch.optim bumps the version counters the caches watch; this covers an optimizer that does not)


def train_seg(model, dataset_loader, optimizer, criterion, num_classes, epoch, device='cuda', use_depth=False, add_criterion=None,
              greenhouse_use_trav=False, weight=1.0):
    """utilities/train_eval_seg.py:16-91 with its own signature (mind the order of the last two arguments: it is not train_seg_ue's);
    returns (miou, average loss) with the SCALAR miou of :84-89 -- `iou.mean() * 100` with greenhouse_use_trav, else
    `iou[[1, 2, 3]].mean() * 100`, an IndexError for num_classes - 1 < 4 as there -- over the epoch's summed areas of the model's one
    output.  There is no flooding.  With the shipped settings (`_single_head_fast_path`: `--model espnetv2` / `espdnet` without depth,
    SegmentationLoss('ce'), momentum SGD) the iterations run on supervised.GraphedSupervisedStep(heads=1) with loss, meters and logit
    gradient taken at the decoder's low-resolution head; the caller's SGD then never steps and holds no state, its groups'
    hyper-parameters are read every iteration, a partial last batch runs eagerly on the same FlatSGD, and a new optimizer object
    starts with zero momentum.  Everything else -- RGB-D batches, an additional criterion with `weight`, an OrderedDict output,
    other models, losses or optimizers -- runs the reference body on the drop-in modules with the caller's optimizer.  Nothing inside
    the loop synchronises (one device-to-host copy per epoch), so the running log line is not printed.  State on the model object as
    for train_seg_ue (release_supervised_loop)."""
    from . import evaluation, supervised
    model.train()
    state = model.__dict__.setdefault('_mspl_supervised_loop', {})
    meters = state.get('meters')
    if meters is None:
        meters = state['meters'] = supervised.SupervisedMeters(num_classes - 1, device)       # MIOU(num_classes - 1), :27
    elif meters.classes != num_classes - 1 or meters.areas.device.type != torch.device(device).type:
        raise RuntimeError('mspl_amd.script.train_seg: this model was run with num_classes=%d on %s before; call '
                           'script.release_supervised_loop(model) first' % (meters.classes + 1, meters.areas.device))
    meters.reset()
    if _single_head_fast_path(model, criterion, optimizer, add_criterion, device, use_depth):
        _train_seg_ue_fast(model, dataset_loader, optimizer, criterion, device, meters, state, heads=1)
    else:
        _train_seg_restated(model, dataset_loader, optimizer, criterion, device, use_depth, add_criterion, weight, meters)
    r = meters.read()                   # the epoch's one device-to-host copy
    iou = r['inter'] / (r['union'] + 1e-10)                                  # :84
    nid_avg = r['extra_sum'] / r['steps'] if (add_criterion is not None and r['steps']) else 0.0
    miou = evaluation.miou_percent(iou, greenhouse_use_trav)                 # :86-89
    print("Epoch: %d[%d steps]\t\tLoss:%.4f\t\tmiou:%.4f\t\tNID loss:%.4f" % (epoch, r['steps'], r['loss_avg'], iou.mean() * 100, nid_avg))
    return miou, r['loss_avg']
