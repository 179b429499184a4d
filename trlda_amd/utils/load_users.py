"""``load_users`` / ``load_users_as_dict`` (reference python/utils/load_users.py): users and their
ratings from a text file of ``uid item rating`` lines, a user's lines grouped together."""
from numpy.random import poisson


def _read_users(filepath, threshold):
    """(uid, [(item, rating), ...]) per run of kept lines with one uid, in file order.  With
    threshold > 0 a rating below it drops the line and the others become 1; a user whose lines
    are all dropped never appears, and the runs on either side of it are joined when their uids
    agree."""
    uid, items = None, []
    with open(filepath) as handle:
        for line in handle:
            u, item, rating = (int(v) for v in line.split())
            if threshold > 0:
                if rating < threshold:
                    continue
                rating = 1
            if u != uid and items:
                yield uid, items
                items = []
            uid = u
            items.append((item, rating))
    if items:
        yield uid, items


def _batches(filepath, batch_size, stochastic, threshold, new, add):
    """The reference's batching: after each user that is not the file's last one, an empty batch
    for every batch size of 0 drawn, then the batch when it holds enough users, then (stochastic)
    a new size; the rest of the users as the last batch.  Sizes are np.random.poisson(batch_size)
    draws, the first when the generator starts."""
    size = poisson(batch_size) if stochastic else batch_size
    batch = new()
    pending = None
    for user in _read_users(filepath, threshold):
        if pending is not None:
            add(batch, pending)
            if batch_size:
                while size == 0:
                    yield []
                    size = poisson(batch_size)
                if len(batch) >= size:
                    yield batch
                    batch = new()
                if stochastic:
                    size = poisson(batch_size)
        pending = user
    if pending is not None:
        add(batch, pending)
    yield batch


def _append(users, user):
    users.append(user[1])


def _store(users, user):
    users[user[0]] = user[1]


def load_users(filepath, batch_size=None, stochastic=False, threshold=4):
    """Loads users from a text file whose lines are ``uid item rating``, grouped by user.  Each user
    is a list of ``(item, rating)`` tuples.  With ``threshold`` > 0, ratings below it are skipped
    and the rest become 1; with ``threshold`` <= 0 ratings are kept as they are.

    Returns a list of users, or with ``batch_size`` a generator of lists of about that many users
    (with ``stochastic=True`` each batch size is a Poisson draw; a draw of 0 yields an empty
    batch).  The lists feed ``update_parameters`` as they are."""
    gen = _batches(filepath, batch_size, stochastic, threshold, list, _append)
    if batch_size:
        return gen
    return next(gen)


def load_users_as_dict(filepath, batch_size=None, stochastic=False, threshold=4):
    """Like ``load_users``, with each batch a dictionary from user id to the user's
    ``(item, rating)`` list (a uid seen again later in a batch keeps its place and takes the later
    list).  An empty batch of a Poisson draw of 0 is an empty list, as in the reference."""
    gen = _batches(filepath, batch_size, stochastic, threshold, dict, _store)
    if batch_size:
        return gen
    return next(gen)
